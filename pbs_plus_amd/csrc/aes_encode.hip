// The AES leg of pbsgpu_blob_encode3_device (include/pbsgpu.h): the encrypted blob kinds written on the
// device. blob.hip plans the call, enqueues the encoder's rounds in front of this leg and its CRC pair behind it, all on one
// stream; this file holds the three kernels in between. The cipher is aes_gcm.h, the code aes_gcm.hip runs:
//   k_aese_head    per blob, one lane: J0 from the staged IV and E_K(J0); the IV goes to bytes 12-27 of the blob.
//   k_aese_pieces  per planned piece of 64 KiB, one workgroup of 256, grid-stride: pbsa::piece_lane with encrypt = true. The
//                  host has planned the pieces for each slot's CAPACITY, the chunk's length; the message's real length is
//                  known only here (res: the encoder's verdict and the frame's length), and a planned piece at or beyond
//                  pieces_of(len) is left alone (piece_len would underflow there; the condition is the workgroup's).
//                  The source is the chunk in src, or the frame where it lies when it won: CTR in place, in == out.
//                  piece_lane allows that: a lane loads its own 16 bytes before it stores them, the tail is one lane's,
//                  byte-exact, and no pointer is __restrict__ (tests/native/test_aes_encode.cpp runs it so on the CPU).
//   k_aese_fold    per blob, one wave: fold_piece over the pieces that ran, tag_of; the tag goes to bytes 28-43 of the blob.
// The key's tables are copied to LDS per workgroup as in k_aes_pieces. Memory instructions: global_* and ds_* only, no
// scratch (tests/test_aes_encode_surface.py). Every pointer a kernel dereferences comes from its arguments.
#include <algorithm>

#include "aes_gcm.h"
#include "engine_internal.h"

using namespace pbse;

namespace pbsk {
namespace aese {

using pbsa::Blk;
using pbsa::KeyTables;

constexpr uint32_t kHdr = PBSGPU_BLOB_HEADER_SIZE;               // magic and CRC: the IV follows
constexpr uint32_t kEncHdr = PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE;  // ... then the tag, then the ciphertext
static_assert(pbsa::kPiece == pbsk::crc::kPiece, "one piece table serves the cipher and the CRC");

// the message of blob i: its length, and whether it is the frame that lies at the blob's data position
struct Shape {
    uint32_t len;
    bool frame;
};
__device__ __forceinline__ Shape shape_of(const uint64_t *res, uint64_t chunk_len, uint32_t i) {
    if (res) {
        const uint64_t r = res[i];
        const uint64_t flen = r & ((1ull << 56) - 1);  // (shorter than the chunk when it won: it lies inside the slot)
        if ((r >> 56) == PBSGPU_BLOB_COMPRESSED) return Shape{(uint32_t)(flen < chunk_len ? flen : chunk_len), true};
    }
    return Shape{(uint32_t)chunk_len, false};
}

__device__ __forceinline__ Blk wave_xor(Blk v) {
    for (int d = 32; d; d >>= 1)
        for (int k = 0; k < 4; ++k) v.w[k] ^= (uint32_t)__shfl_xor((int)v.w[k], d, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_aese_head(const KeyTables *kt, const uint8_t *ivs, uint8_t *dst, const uint64_t *doff,
                                                   uint32_t n, Blk *heads) {
    __shared__ uint32_t te0[256];
    te0[threadIdx.x] = kt->te0[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint8_t *iv = ivs + 16ull * i;
    const Blk j0 = pbsa::j0_of(kt->h, iv, 16);
    heads[2 * i] = j0;
    heads[2 * i + 1] = pbsa::encrypt_block(kt->rk, te0, j0);
    pbsa::store_be(dst + doff[i] + kHdr, pbsa::load_be_part(iv, 16));
}

__global__ __launch_bounds__(256) void k_aese_pieces(const KeyTables *kt, const uint8_t *src, uint8_t *dst,
                                                     const pbsgpu_segment *segs, const uint64_t *doff, const uint64_t *res,
                                                     const uint64_t *pbase, const uint32_t *pseg, uint32_t npieces,
                                                     const Blk *heads, Blk *partials) {
    static_assert(pbsa::kStride == 256, "one lane of the piece per thread");
    __shared__ uint32_t te0[256];
    __shared__ uint32_t red[256];
    __shared__ Blk stride[256];
    __shared__ Blk box[4];
    te0[threadIdx.x] = kt->te0[threadIdx.x];
    red[threadIdx.x] = kt->red[threadIdx.x];
    stride[threadIdx.x] = kt->stride[threadIdx.x];
    __syncthreads();
    for (uint32_t p = blockIdx.x; p < npieces; p += gridDim.x) {
        const uint32_t i = pseg[p];
        const uint32_t piece = (uint32_t)(p - pbase[i]);
        const pbsgpu_segment sg = segs[i];
        const Shape sh = shape_of(res, sg.length, i);
        if (piece >= pbsa::pieces_of(sh.len)) continue;  // (the workgroup's: planned for the capacity, past the message's end)
        const uint64_t at = (uint64_t)piece * pbsa::kPiece;
        uint8_t *out = dst + doff[i] + kEncHdr + at;
        const uint8_t *in = sh.frame ? out : src + sg.offset + at;
        Blk y = pbsa::piece_lane(kt->rk, te0, stride, red, kt->low, heads[2 * i], piece, in, out, pbsa::piece_len(sh.len, piece),
                                 true, threadIdx.x);
        y = wave_xor(y);
        if ((threadIdx.x & 63u) == 0) box[threadIdx.x >> 6] = y;
        __syncthreads();
        if (threadIdx.x == 0) partials[p] = pbsa::bxor(pbsa::bxor(box[0], box[1]), pbsa::bxor(box[2], box[3]));
        __syncthreads();  // the box goes to the next piece
    }
}

__global__ __launch_bounds__(64) void k_aese_fold(const KeyTables *kt, uint8_t *dst, const pbsgpu_segment *segs, const uint64_t *doff,
                                                 const uint64_t *res, const uint64_t *pbase, uint32_t n, const Blk *heads,
                                                 const Blk *partials) {
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t len = shape_of(res, segs[i].length, i).len;
        const uint32_t np = pbsa::pieces_of(len);
        const Blk *part = partials + pbase[i];
        Blk terms{{0, 0, 0, 0}};
        for (uint32_t p = threadIdx.x; p < np; p += 64) terms = pbsa::bxor(terms, pbsa::fold_piece(part[p], len, p, kt->pow2));
        terms = wave_xor(terms);
        if (threadIdx.x == 0) pbsa::store_be(dst + doff[i] + kHdr + 16, pbsa::tag_of(terms, len, kt->h, heads[2 * i + 1]));
    }
}

int enqueue(pbsgpu_engine *e, Slot *s, const pbsgpu_aes_key *key, const Job &job, const uint8_t *ivs) {
    const uint32_t n = job.nseg;
    const uint8_t *divs = nullptr;
    CHK(put_table(s, ivs, (size_t)n * 16, &divs));
    Blk *heads = s->take<Blk>((size_t)n * 2);
    Blk *partials = s->take<Blk>((size_t)job.npieces + 1);
    CHK(s->taken());
    const KeyTables *kt = static_cast<const KeyTables *>(pbsk::aes::key_tables(key));
    hipLaunchKernelGGL(k_aese_head, dim3((n + 255) / 256), dim3(256), 0, s->stream, kt, divs, job.dst, job.doff, n, heads);
    HIPCHK(hipGetLastError());
    if (job.npieces) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(job.npieces, (uint64_t)e->num_cus * 8);
        hipLaunchKernelGGL(k_aese_pieces, dim3(grid), dim3(256), 0, s->stream, kt, job.src, job.dst, job.segs, job.doff, job.res,
                           job.pbase, job.pseg, job.npieces, heads, partials);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_aese_fold, dim3(std::min<uint32_t>(n, (uint32_t)e->num_cus * 16)), dim3(64), 0, s->stream, kt, job.dst,
                       job.segs, job.doff, job.res, job.pbase, n, heads, partials);
    HIPCHK(hipGetLastError());
    return PBSGPU_OK;
}

}  // namespace aese
}  // namespace pbsk
