// What the block kernels of the zstd encoder share (zstd_encode.hip: k_zenc_blocks, predefined tables and explicit
// offsets; zstd_encode_tables.hip: k_zenc_tblocks, per-block tables and repeat codes; zstd_encode_window.hip:
// k_zenc_wblocks and k_zenc_wtblocks, the same two with the long-range match finder): the plan of a round, the lanes'
// policy, and the loop over the round's blocks. The first two differ in the State they hold in LDS and in nothing else:
// same grid, same job sources, same scratch, same result word per block, and k_zenc_assemble serves all four. The window
// kernels keep the match finder's table in the workgroup's part of the scratch and read a chunk in two parts where it
// lies, through enc::Src2, instead of staging the block that holds the seam: the seam may lie anywhere in the history.
#pragma once

#include "engine_internal.h"
#include "zstd_encode.h"

namespace pbsk {
namespace zenc {

namespace ze = pbsz::enc;

struct Plan {
    const uint8_t *src;
    const Job *jobs;         // every chunk of the call
    const uint32_t *bchunk;  // every block of the call: its chunk
    uint8_t *blkout;         // the round's blocks, kBlockMax bytes each
    uint32_t *bres;          // the round's blocks: type | size << 2
    uint64_t *boff;          // the round's blocks: where the block header goes in its frame
    uint8_t *lit;            // per workgroup of k_zenc_blocks: kBlockMax
    uint64_t *seqs;          // per workgroup: kSeqCap
    uint8_t *stage;          // per workgroup: kBlockMax, when a job may have two parts
    uint8_t *dst;
    uint64_t *res;           // per Job::out: frame length | status << 56
    uint32_t *next;          // the round's block counter, zero at its start
    uint32_t b0, b1, c0, c1; // the round
    uint32_t blob;
    uint32_t window_log;     // the window kernels: pbsgpu_engine_options::zstd_window_log. Their scratch is one piece of
                             // kWindowWork bytes per workgroup from `lit` on: literals, sequences, the match finder's table
    const uint64_t *sums;    // per Job::out: XXH64(content, 0), for k_zenc_assemble to close the frame with its low word
                             // (pbsgpu_zstd_encode2_device with PBSGPU_ZSTD_F_CHECKSUM); nullptr: frames without a checksum
};
constexpr size_t kWindowWork = (size_t)pbsz::kBlockMax + (size_t)ze::kSeqCap * 8 + (sizeof(uint32_t) << ze::kWindowHashLog);

// where byte p of the chunk lies, as an offset from Plan::src
__device__ __forceinline__ uint64_t chunk_byte(const Job &j, uint32_t p) {
    return p < j.a ? j.src_off + p : j.src1_off + (p - j.a);
}

struct WaveLanes {
    static __device__ __forceinline__ int lane() {
        int x = (int)threadIdx.x;
        asm volatile("" : "+v"(x));  // taken anew at every use
        return x;
    }
    static __device__ __forceinline__ int lanes() { return 64; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
    static __device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    static __device__ __forceinline__ void amax(uint32_t *p, uint32_t v) { atomicMax(p, v); }
    static __device__ __forceinline__ void aadd(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
};

// One workgroup of 64: the round's blocks from the counter, one at a time, each through encode_block on `st` (LDS).
template <class S>
__device__ __forceinline__ void encode_blocks(const Plan &pl, S &st) {
    bool tables = false;
    uint8_t *lit = pl.lit + (uint64_t)blockIdx.x * (S::kWindow ? kWindowWork : (size_t)pbsz::kBlockMax);
    uint64_t *seqs = S::kWindow ? reinterpret_cast<uint64_t *>(lit + pbsz::kBlockMax) : pl.seqs + (uint64_t)blockIdx.x * ze::kSeqCap;
    for (;;) {
        uint32_t b = 0;  // the round's next block: blocks differ in cost, and the device's plan leaves some out altogether
        if (threadIdx.x == 0) b = atomicAdd(pl.next, 1u);
        b = pl.b0 + WaveLanes::uni(b);
        if (b >= pl.b1) break;
        const Job j = pl.jobs[pl.bchunk[b]];  // (uniform addresses: scalar loads)
        if (j.out == kNoJob) continue;        // a chunk the device's plan does not encode
        if (!tables) {
            ze::init_tables<WaveLanes>(st);
            tables = true;
        }
        const uint32_t at = (b - j.first) * pbsz::kBlockMax;
        const uint32_t bn = j.len - at < pbsz::kBlockMax ? j.len - at : pbsz::kBlockMax;
        uint8_t *blk = pl.blkout + (uint64_t)(b - pl.b0) * pbsz::kBlockMax;
        if constexpr (S::kWindow) {  // the block behind its history, hn bytes of the chunk, from where the two parts lie
            const uint32_t hn = at < (1u << pl.window_log) ? at : 1u << pl.window_log, w0 = at - hn;
            const uint8_t *p1 = pl.src + j.src1_off;
            const ze::Src2 content = w0 < j.a ? ze::Src2{pl.src + j.src_off + w0, p1, j.a - w0} : ze::Src2{p1 + (w0 - j.a), p1 + (w0 - j.a), 0u};
            uint32_t *wtab = reinterpret_cast<uint32_t *>(lit + pbsz::kBlockMax + (size_t)ze::kSeqCap * 8);
            const uint32_t r = ze::encode_block<WaveLanes, S>(st, content, bn, blk, lit, seqs, hn, wtab);
            if (threadIdx.x == 0) pl.bres[b - pl.b0] = r;
            __syncthreads();  // State, the literals, the sequences and the table go to the next block
            continue;
        }
        const uint8_t *content = pl.src + chunk_byte(j, at);
        if (at < j.a && j.a < at + bn) {  // the one block of a chunk that holds the seam between its parts: put together first
            uint8_t *sg = pl.stage + (uint64_t)blockIdx.x * pbsz::kBlockMax;
            for (uint32_t i = threadIdx.x; i < bn; i += 64) sg[i] = pl.src[chunk_byte(j, at + i)];
            __syncthreads();
            content = sg;
        }
        const uint32_t r = ze::encode_block<WaveLanes, S>(st, content, bn, blk, lit, seqs);
        if (threadIdx.x == 0) pl.bres[b - pl.b0] = r;
        __syncthreads();  // State, the literals, the sequences and the staged block go to the next block
    }
}

// zstd_encode_tables.hip: the block kernel of the mode with tables (pbsgpu_engine_options::zstd_seq_tables = 1)
hipError_t launch_blocks_tables(const Plan &pl, uint32_t grid, hipStream_t st);
// zstd_encode_window.hip: the block kernels of the long-range match finder (pbsgpu_engine_options::zstd_window_log != 0),
// without and with tables
hipError_t launch_blocks_window(const Plan &pl, uint32_t grid, bool tables, hipStream_t st);

}  // namespace zenc
}  // namespace pbsk
