// Data blobs (pbsgpu_crc32_* / pbsgpu_blob_*, include/pbsgpu.h): the CRC-32 of many byte ranges, the uncompressed blob a
// PBS server takes as a chunk upload, and the chunk check of the read side (magic, CRC, size, SHA-256).
//
// CRC-32/ISO-HDLC in the reflected form: a 32-bit word c stands for a polynomial of degree < 32 with bit 31 - i the
// coefficient of x^i (x^0 = 0x80000000). raw(M) is the register after M with init 0 and no final xor; it is linear:
//   raw(A || B) = raw(A) * x^(8|B|) + raw(B)            (mod P, GF(2))
//   crc(M)      = raw(M) + 0xFFFFFFFF * x^(8|M|) + 0xFFFFFFFF
// and leading zero bytes do not change raw(). gfx950 has no carry-less multiply in the VALU: products are 32 conditional
// xor-shift steps (mul below), and the byte-wise work is table lookups from LDS.
//
// Two kernels over a host plan (the shape of k_xxh3_sums + k_xxh3):
//   k_crc_pieces  every segment is cut into pieces of kPiece = 64 KiB aligned at the segment's END (only the first piece
//                 of a segment is short); one wave per piece. The piece is seen as rows of kRow = 1024 bytes, zero-padded
//                 in FRONT to whole rows (raw() unchanged). In row r, lane l owns the 16 bytes at 1024 r + 16 l: one
//                 coalesced 1 KiB load per row and wave. A lane runs slice-by-16 over the stream
//                 S_l = blk(0,l) 0^1008 blk(1,l) 0^1008 ...: its 16 tables T_m[b] = raw(b) * x^(8 (m + 1008)) fold the
//                 1008 bytes of the other lanes into the lookup, so a row costs a lane 16 LDS reads, as plain
//                 slice-by-16 does. The piece is then raw(piece) = sum_l raw(S_l) * x^(-128 l) (x is invertible mod P):
//                 one product per lane and a wave-wide xor.
//                 The init value is folded in here too: the segment's first four bytes enter the CRC inverted, which
//                 adds 0xFFFFFFFF * x^(8|M|) (segments of 1-3 bytes take that term in the fold instead).
//   k_crc_fold    one wave per segment: its pieces right to left in blocks of 64 lanes, a 6-level xor tree whose left
//                 halves are shifted by x^(8 kPiece 2^k) (the right half of every merge holds only whole pieces, since
//                 the short piece is the segment's first), then Horner over the blocks; final xor; the blob header.
// The encode pass is the same pair with a destination: the piece kernel stores every loaded row at the blob's data
// position (arbitrary alignment, one row and lane at a time) and the fold writes the 12-byte header.
// The ring's two-part chunks (k_pagecrc_*) and the restore (k_dec_*) have plans and kernels of their own, but one body:
// piece_raw is the one walk over a piece, with three forms of the store (the whole piece if there is a destination, the
// whole piece, the piece clipped to a byte range); a piece kernel only finds its piece's bytes, destination and inverted
// head in its plan. The folds share fold_part, finish and store_header in the same way, the copies copy_bytes.
// Memory instructions: global_* only (address-space-1 pointers); no scratch (tests/test_blob_surface.py).
#include "ring_internal.h"

using namespace pbse;

namespace pbsk {
namespace crc {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr uint32_t kOne = 0x80000000u;  // x^0
constexpr uint32_t kXInv = ((kPoly << 1) & 0xffffffffu) | 1u;  // x^-1 = (P - 1) / x
constexpr uint32_t kRow = 1024;
constexpr uint32_t kGap = kRow - 16;
constexpr uint32_t kFoldLanes = 64;
static_assert(kPieceLog == kBlobPieceLog, "ring.cpp bounds the piece count with this");

__host__ __device__ constexpr uint32_t mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
    }
    return p;
}

struct Consts {
    uint32_t x8[64];     // x^(8 * 2^j)
    uint32_t klane[64];  // x^(-128 l): lane l's share of a piece
    uint32_t small[4];   // x^(8 L), L < 4
    uint32_t gap;        // x^(8 kGap)
};

__host__ __device__ constexpr uint32_t pow_from(const uint32_t (&x8)[64], uint64_t bytes) {  // x^(8 bytes)
    uint32_t r = kOne;
    for (int j = 0; j < 64; ++j)
        if ((bytes >> j) & 1u) r = mul(r, x8[j]);
    return r;
}

constexpr Consts make_consts() {
    Consts c{};
    uint32_t x = 1u << 30;  // x^1
    for (int i = 0; i < 3; ++i) x = mul(x, x);  // x^8
    for (int j = 0; j < 64; ++j) {
        c.x8[j] = x;
        x = mul(x, x);
    }
    uint32_t inv128 = kXInv;
    for (int i = 0; i < 7; ++i) inv128 = mul(inv128, inv128);  // x^-128
    c.klane[0] = kOne;
    for (int l = 1; l < 64; ++l) c.klane[l] = mul(c.klane[l - 1], inv128);
    for (int l = 0; l < 4; ++l) c.small[l] = pow_from(c.x8, (uint64_t)l);
    c.gap = pow_from(c.x8, kGap);
    return c;
}

__device__ constexpr Consts kDev = make_consts();
constexpr Consts kHost = make_consts();

// the plan one launch pair works on (host-built, device arrays)
struct Plan {
    const uint8_t *src;
    const pbsgpu_segment *segs;  // nseg ranges of src
    const uint64_t *pbase;       // nseg + 1: index of each segment's first piece
    const uint32_t *pseg;        // npieces: segment of each piece
    uint32_t *praw;              // npieces: raw CRC of each piece
    uint32_t *crcs;              // nseg: the result
    uint8_t *dst;                // encode: blobs (nullptr: CRC only)
    const uint64_t *doff;        // encode: offset of blob i in dst
    uint64_t npieces;
    uint32_t nseg;
    uint32_t magic_lo, magic_hi;  // encode: the header's magic (little endian words)
};

// every access goes through a global-address-space pointer: a generic one compiles to flat_* 
#define CRC_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef const CRC_GLOBAL uint8_t *gbyte_ptr;
typedef const CRC_GLOBAL uint32_t *gword_ptr;
typedef const CRC_GLOBAL uint64_t *gquad_ptr;
typedef const CRC_GLOBAL u32x4_a4 *gvec4_ptr;
typedef CRC_GLOBAL uint8_t *gbyte_out;
typedef CRC_GLOBAL uint16_t *ghalf_out;
typedef CRC_GLOBAL uint32_t *gword_out;
typedef CRC_GLOBAL u32x3_a4 *gvec3_out;
typedef CRC_GLOBAL u32x4_a4 *gvec4_out;

// 16 bytes at q; s = q & 3 (wave-uniform: every lane's q has the same alignment). The dwords read are the ones that hold
// a byte of [q, q + 16), so nothing outside the pages of the range is touched.
__device__ __forceinline__ void load16(const uint8_t *q, uint32_t s, uint32_t (&w)[4]) {
    const gvec4_ptr a = (gvec4_ptr)(q - s);
    const u32x4_a4 t = a[0];
    if (s == 0) {
        w[0] = t.x;
        w[1] = t.y;
        w[2] = t.z;
        w[3] = t.w;
    } else {
        const uint32_t e = ((gword_ptr)(q - s))[4];
        w[0] = __builtin_amdgcn_alignbyte(t.y, t.x, s);
        w[1] = __builtin_amdgcn_alignbyte(t.z, t.y, s);
        w[2] = __builtin_amdgcn_alignbyte(t.w, t.z, s);
        w[3] = __builtin_amdgcn_alignbyte(e, t.w, s);
    }
}

// 16 bytes to o; s = o & 3 (wave-uniform): head bytes up to a dword boundary, three (or four) aligned dwords, tail bytes
__device__ __forceinline__ void store16(uint8_t *o, uint32_t s, const uint32_t (&w)[4]) {
    if (s == 0) {
        u32x4_a4 v;
        v.x = w[0];
        v.y = w[1];
        v.z = w[2];
        v.w = w[3];
        *(gvec4_out)o = v;
        return;
    }
    const uint32_t h = 4 - s;  // head bytes
    u32x3_a4 v;
    v.x = __builtin_amdgcn_alignbyte(w[1], w[0], h);
    v.y = __builtin_amdgcn_alignbyte(w[2], w[1], h);
    v.z = __builtin_amdgcn_alignbyte(w[3], w[2], h);
    if (h & 1) ((gbyte_out)o)[0] = (uint8_t)w[0];
    if (h & 2) *(ghalf_out)(o + (h & 1)) = (uint16_t)(w[0] >> (8 * (h & 1)));
    *(gvec3_out)(o + h) = v;
    const uint32_t t = w[3] >> (8 * h);  // the last s bytes
    if (s & 2) *(ghalf_out)(o + 12 + h) = (uint16_t)t;
    if (s & 1) ((gbyte_out)o)[15] = (uint8_t)(t >> (8 * (s & 2)));
}

// one row of a lane's stream: c = raw(S) after 16 more bytes and the 1008 of the other lanes
__device__ __forceinline__ uint32_t step(const uint32_t (*tab)[256], uint32_t c, const uint32_t (&w)[4]) {
    const uint32_t t = c ^ w[0];
    return tab[15][t & 255] ^ tab[14][(t >> 8) & 255] ^ tab[13][(t >> 16) & 255] ^ tab[12][t >> 24] ^
           tab[11][w[1] & 255] ^ tab[10][(w[1] >> 8) & 255] ^ tab[9][(w[1] >> 16) & 255] ^ tab[8][w[1] >> 24] ^
           tab[7][w[2] & 255] ^ tab[6][(w[2] >> 8) & 255] ^ tab[5][(w[2] >> 16) & 255] ^ tab[4][w[2] >> 24] ^
           tab[3][w[3] & 255] ^ tab[2][(w[3] >> 8) & 255] ^ tab[1][(w[3] >> 16) & 255] ^ tab[0][w[3] >> 24];
}

// a lane's 16 bytes at piece position pos, as found, in the rows that need care: padding in front of the piece reads as
// zeros (pos < 0), and the lane that straddles the piece's start goes byte by byte
// (load and inversion are two helpers although piece_raw alone calls them: the store between them takes the bytes as found,
// and a fused load-store-invert is what each kernel once had to undo by hand)
struct Row {
    uint32_t w[4];
};
__device__ __forceinline__ Row row_edge(const uint8_t *d, int32_t pos, uint32_t sd) {
    Row x{{0, 0, 0, 0}};
    if (pos >= 0) {
        load16(d + pos, sd, x.w);
    } else if (pos > -16) {
#pragma unroll
        for (int j = 0; j < 16; ++j)  // (fixed bounds: the words stay in registers)
            if (pos + j >= 0) x.w[j >> 2] |= (uint32_t)((gbyte_ptr)d)[pos + j] << (8 * (j & 3));
    }
    return x;
}

// bytes [0, inv) of the piece are among the first four of what the CRC covers: they enter inverted (the init value)
__device__ __forceinline__ void invert_head(uint32_t (&w)[4], int32_t pos, uint32_t inv) {
    if (pos < (int32_t)inv) {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (pos + j >= 0 && pos + j < (int32_t)inv) w[j >> 2] ^= 0xffu << (8 * (j & 3));
    }
}

// a lane's 16 bytes at piece position pos, of which [a, b) may be stored (piece coordinates; so = (o + pos) & 3)
__device__ __forceinline__ void store_clip(uint8_t *o, uint32_t so, int32_t pos, int32_t a, int32_t b,
                                           const uint32_t (&w)[4]) {
    if (pos >= a && pos + 16 <= b) {
        store16(o + pos, so, w);
    } else if (pos + 16 > a && pos < b) {
#pragma unroll
        for (int j = 0; j < 16; ++j)  // (fixed bounds: the words stay in registers)
            if (pos + j >= a && pos + j < b) ((gbyte_out)o)[pos + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}

// What the piece walk does with the bytes it has loaded, in three forms. `o` is where piece position 0 goes; edge() takes
// a lane of the rows that may hold padding (signed position), row() a lane of a whole row (the offset stays unsigned: a
// signed one costs the encode kernels a wave of occupancy).
struct PutAll {  // the whole piece
    uint8_t *o;
    __device__ __forceinline__ void edge(uint32_t so, int32_t pos, const uint32_t (&w)[4]) const {
        store_clip(o, so, pos, 0, INT32_MAX, w);
    }
    __device__ __forceinline__ void row(uint32_t so, uint32_t pos, const uint32_t (&w)[4]) const { store16(o + pos, so, w); }
};
struct PutIf {  // the whole piece when there is a destination
    uint8_t *o;
    __device__ __forceinline__ void edge(uint32_t so, int32_t pos, const uint32_t (&w)[4]) const {
        if (o) PutAll{o}.edge(so, pos, w);
    }
    __device__ __forceinline__ void row(uint32_t so, uint32_t pos, const uint32_t (&w)[4]) const {
        if (o) PutAll{o}.row(so, pos, w);
    }
};
struct PutClip {  // the piece's bytes [a, b) when there is a destination
    uint8_t *o;
    int32_t a, b;
    __device__ __forceinline__ void edge(uint32_t so, int32_t pos, const uint32_t (&w)[4]) const {
        if (o) store_clip(o, so, pos, a, b, w);
    }
    __device__ __forceinline__ void row(uint32_t so, uint32_t pos, const uint32_t (&w)[4]) const { edge(so, (int32_t)pos, w); }
};

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    return v;
}

// tab[m] = T_m (m = 0..15), tab[16] = the byte table raw(b); one entry of each per thread of the workgroup
__device__ __forceinline__ void build_tables(uint32_t (*tab)[256]) {
    const uint32_t b = threadIdx.x;
    uint32_t c = b;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (kPoly & (0u - (c & 1u)));
    tab[16][b] = c;
    uint32_t t = mul(c, kDev.gap);
    tab[0][b] = t;
    __syncthreads();
    for (int m = 1; m < 16; ++m) {  // one more zero byte: the plain CRC step
        t = (t >> 8) ^ tab[16][t & 255];
        tab[m][b] = t;
    }
    __syncthreads();
}

// One wave's walk over a piece: raw CRC of the n bytes at d, of which the first inv enter inverted, every loaded row
// handed to put. The same value in every lane.
template <class Put>
__device__ __forceinline__ uint32_t piece_raw(const uint32_t (*tab)[256], const uint8_t *d, uint32_t n, uint32_t inv,
                                              uint32_t lane, const Put &put) {
    const uint32_t rows = (n + kRow - 1) / kRow;
    const uint32_t z = rows * kRow - n;  // zero bytes in front of the piece
    const uint32_t sd = (uint32_t)((uintptr_t)d - z) & 3u;
    const uint32_t so = (uint32_t)((uintptr_t)put.o - z) & 3u;
    uint32_t c = 0;
    const auto edge = [&](int32_t pos) __attribute__((always_inline)) {
        const Row x = row_edge(d, pos, sd);
        Row y = x;
        invert_head(y.w, pos, inv);
        c = step(tab, c, y.w);   // (the table reads are in flight while the store, which takes the bytes as found, goes out)
        put.edge(so, pos, x.w);
    };
    edge((int32_t)(16 * lane) - (int32_t)z);
    uint32_t r = 1;
    if (z > kRow - 4 && rows > 1) {  // the inverted bytes reach into row 1
        edge((int32_t)(kRow + 16 * lane) - (int32_t)z);
        r = 2;
    }
    for (; r + 4 <= rows; r += 4) {
        uint32_t w[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) load16(d + (r + k) * kRow + 16 * lane - z, sd, w[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            put.row(so, (r + k) * kRow + 16 * lane - z, w[k]);
            c = step(tab, c, w[k]);
        }
    }
    for (; r < rows; ++r) {
        uint32_t w[4];
        load16(d + r * kRow + 16 * lane - z, sd, w);
        put.row(so, r * kRow + 16 * lane - z, w);
        c = step(tab, c, w);
    }
    return wave_xor(mul(c, kDev.klane[lane]));
}

__global__ __launch_bounds__(256) void k_crc_pieces(Plan pl) {
    __shared__ uint32_t tab[17][256];
    build_tables(tab);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    for (uint64_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); p < pl.npieces; p += nw) {
        const uint32_t i = ((gword_ptr)pl.pseg)[p];
        const uint64_t b0 = ((gquad_ptr)pl.pbase)[i];
        const uint64_t m = ((gquad_ptr)pl.pbase)[i + 1] - b0;
        const pbsgpu_segment sg{((gquad_ptr)pl.segs)[2 * i], ((gquad_ptr)pl.segs)[2 * i + 1]};
        const uint64_t hi = sg.length - (m - 1 - (p - b0)) * kPiece;  // piece = segment bytes [lo, hi)
        const uint64_t lo = hi > kPiece ? hi - kPiece : 0;
        uint8_t *o = pl.dst ? pl.dst + ((gquad_ptr)pl.doff)[i] + PBSGPU_BLOB_HEADER_SIZE + lo : nullptr;
        const uint32_t inv = (sg.length >= 4 && lo < 4) ? (uint32_t)((hi < 4 ? hi : 4) - lo) : 0u;
        const uint32_t v = piece_raw(tab, pl.src + sg.offset + lo, (uint32_t)(hi - lo), inv, lane, PutIf{o});
        if (lane == 0) ((gword_out)pl.praw)[p] = v;
    }
}

// raw CRC of one range from its m >= 1 pieces: right to left in blocks of 64 lanes, a 6-level xor tree, Horner over the
// blocks (only the first piece is short, so the right half of every merge holds whole pieces)
__device__ __forceinline__ uint32_t fold_part(gword_ptr raw, uint32_t m, uint32_t lane) {
    if (m == 1) return raw[0];
    uint32_t acc = 0;
    for (uint32_t blk = (m - 1) / kFoldLanes + 1; blk-- > 0;) {  // left to right
        const uint32_t q = blk * kFoldLanes + lane;              // q = pieces from the range's end
        uint32_t v = q < m ? raw[m - 1 - q] : 0u;
#pragma unroll
        for (int lv = 0; lv < 6; ++lv) {  // the lane with bit lv clear holds the right (later) half
            const uint32_t u = __shfl_xor(v, 1 << lv, 64);
            if (!(lane & (1u << lv))) v ^= mul(u, kDev.x8[kPieceLog + lv]);
        }
        acc = mul(acc, kDev.x8[kPieceLog + 6]) ^ __shfl(v, 0, 64);
    }
    return acc;
}

// raw -> CRC: the init term that the piece pass leaves to the fold (lengths under 4), and the final xor
__device__ __forceinline__ uint32_t finish(uint32_t acc, uint64_t len) {
    return (len < 4 ? acc ^ mul(0xffffffffu, kDev.small[len]) : acc) ^ 0xffffffffu;
}

// the 12-byte blob header at h, one byte per lane
__device__ __forceinline__ void store_header(uint8_t *h, uint32_t lane, uint32_t magic_lo, uint32_t magic_hi, uint32_t crc) {
    if (lane < PBSGPU_BLOB_HEADER_SIZE) {
        const uint32_t word = lane < 4 ? magic_lo : lane < 8 ? magic_hi : crc;
        ((gbyte_out)h)[lane] = (uint8_t)(word >> (8 * (lane & 3)));
    }
}

__global__ __launch_bounds__(256) void k_crc_fold(Plan pl) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    for (uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); i < pl.nseg; i += nw) {
        const uint64_t b0 = ((gquad_ptr)pl.pbase)[i];
        const uint32_t m = (uint32_t)(((gquad_ptr)pl.pbase)[i + 1] - b0);  // (the host refuses 2^32 pieces)
        const uint32_t acc = m ? fold_part((gword_ptr)pl.praw + b0, m, lane) : 0u;
        const uint32_t crc = finish(acc, ((gquad_ptr)pl.segs)[2 * i + 1]);
        if (lane == 0) ((gword_out)pl.crcs)[i] = crc;
        if (pl.dst) store_header(pl.dst + ((gquad_ptr)pl.doff)[i], lane, pl.magic_lo, pl.magic_hi, crc);
    }
}

// ---- blobs whose kind the device decides (pbsgpu_blob_encode2_device with PBSGPU_ENCODE_F_ZSTD) -------------
// zstd_encode.hip has left, per chunk, its verdict and the frame's length (res), and has written the frames that won at
// their blobs' data positions. The CRC then covers the frame where it lies (no store), or the chunk, which the walk
// copies as the plain encode does. The pieces are planned on the host for each slot's capacity, the chunk's length; the
// range actually covered is known only here, and the planned pieces past its end do nothing. Same walk, same fold.
struct Enc2Plan {
    Plan p;
    const uint64_t *res;  // nseg: frame length | kind << 56
    uint32_t *lens;       // nseg: the blob's length
    uint8_t *kinds;       // nseg
    uint32_t zmagic_lo, zmagic_hi;  // the compressed kind's magic
};

__global__ __launch_bounds__(256) void k_enc2_pieces(Enc2Plan pl) {
    __shared__ uint32_t tab[17][256];
    build_tables(tab);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    for (uint64_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); p < pl.p.npieces; p += nw) {
        const uint32_t i = ((gword_ptr)pl.p.pseg)[p];
        const uint64_t b0 = ((gquad_ptr)pl.p.pbase)[i];
        const pbsgpu_segment sg{((gquad_ptr)pl.p.segs)[2 * i], ((gquad_ptr)pl.p.segs)[2 * i + 1]};
        const uint64_t res = ((gquad_ptr)pl.res)[i];
        const bool comp = (res >> 56) == PBSGPU_BLOB_COMPRESSED;
        const uint64_t len = comp ? res & ((1ull << 56) - 1) : sg.length;  // comp: shorter than the chunk
        const uint64_t m = (len + kPiece - 1) >> kPieceLog;
        if (p - b0 >= m) continue;  // (wave-uniform)
        const uint64_t hi = len - (m - 1 - (p - b0)) * kPiece;
        const uint64_t lo = hi > kPiece ? hi - kPiece : 0;
        uint8_t *data = pl.p.dst + ((gquad_ptr)pl.p.doff)[i] + PBSGPU_BLOB_HEADER_SIZE;
        const uint8_t *from = comp ? data : pl.p.src + sg.offset;
        const uint32_t inv = (len >= 4 && lo < 4) ? (uint32_t)((hi < 4 ? hi : 4) - lo) : 0u;
        const uint32_t v = piece_raw(tab, from + lo, (uint32_t)(hi - lo), inv, lane, PutIf{comp ? nullptr : data + lo});
        if (lane == 0) ((gword_out)pl.p.praw)[p] = v;
    }
}

__global__ __launch_bounds__(256) void k_enc2_fold(Enc2Plan pl) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    for (uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); i < pl.p.nseg; i += nw) {
        const uint64_t b0 = ((gquad_ptr)pl.p.pbase)[i];
        const uint64_t res = ((gquad_ptr)pl.res)[i];
        const bool comp = (res >> 56) == PBSGPU_BLOB_COMPRESSED;
        const uint64_t len = comp ? res & ((1ull << 56) - 1) : ((gquad_ptr)pl.p.segs)[2 * i + 1];
        const uint32_t m = (uint32_t)((len + kPiece - 1) >> kPieceLog);
        const uint32_t acc = m ? fold_part((gword_ptr)pl.p.praw + b0, m, lane) : 0u;
        const uint32_t crc = finish(acc, len);
        if (lane == 0) {
            ((gword_out)pl.p.crcs)[i] = crc;
            ((gword_out)pl.lens)[i] = (uint32_t)(len + PBSGPU_BLOB_HEADER_SIZE);
            ((gbyte_out)pl.kinds)[i] = comp ? PBSGPU_BLOB_COMPRESSED : PBSGPU_BLOB_UNCOMPRESSED;
        }
        store_header(pl.p.dst + ((gquad_ptr)pl.p.doff)[i], lane, comp ? pl.zmagic_lo : pl.p.magic_lo,
                     comp ? pl.zmagic_hi : pl.p.magic_hi, crc);
    }
}

// ---- the encrypted kinds (pbsgpu_blob_encode3_device with PBSGPU_ENCODE_F_AES) -----------------------------
// aes_encode.hip has left, per blob, IV, tag and ciphertext behind the 12 header bytes; the CRC covers the ciphertext where
// it lies, so the walk stores nothing. With F_ZSTD the ciphertext is as long as the frame when the frame won (res, as
// above), else as long as the chunk; the pieces are planned for the chunk's length and the ones past the end do nothing.
struct Enc3Plan {
    Plan p;               // p.src is not read; p.magic_*: the encrypted kind's
    const uint64_t *res;  // nseg: frame length | kind << 56, or nullptr: nothing was compressed
    uint32_t *lens;       // nseg: the blob's length
    uint8_t *kinds;       // nseg
    uint32_t zmagic_lo, zmagic_hi;  // the encrypted-compressed kind's magic
};

// the ciphertext's length of blob i, and whether it holds a frame
__device__ __forceinline__ uint64_t enc3_len(const Enc3Plan &pl, uint32_t i, bool *comp) {
    const uint64_t chunk = ((gquad_ptr)pl.p.segs)[2 * i + 1];
    const uint64_t res = pl.res ? ((gquad_ptr)pl.res)[i] : 0;
    *comp = (res >> 56) == PBSGPU_BLOB_COMPRESSED;
    const uint64_t flen = res & ((1ull << 56) - 1);
    return *comp && flen < chunk ? flen : chunk;  // (a frame that won is shorter than the chunk)
}

__global__ __launch_bounds__(256) void k_enc3_pieces(Enc3Plan pl) {
    __shared__ uint32_t tab[17][256];
    build_tables(tab);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    for (uint64_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); p < pl.p.npieces; p += nw) {
        const uint32_t i = ((gword_ptr)pl.p.pseg)[p];
        const uint64_t b0 = ((gquad_ptr)pl.p.pbase)[i];
        bool comp;
        const uint64_t len = enc3_len(pl, i, &comp);
        const uint64_t m = (len + kPiece - 1) >> kPieceLog;
        if (p - b0 >= m) continue;  // (wave-uniform)
        const uint64_t hi = len - (m - 1 - (p - b0)) * kPiece;
        const uint64_t lo = hi > kPiece ? hi - kPiece : 0;
        const uint8_t *data = pl.p.dst + ((gquad_ptr)pl.p.doff)[i] + PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE;
        const uint32_t inv = (len >= 4 && lo < 4) ? (uint32_t)((hi < 4 ? hi : 4) - lo) : 0u;
        const uint32_t v = piece_raw(tab, data + lo, (uint32_t)(hi - lo), inv, lane, PutIf{nullptr});
        if (lane == 0) ((gword_out)pl.p.praw)[p] = v;
    }
}

__global__ __launch_bounds__(256) void k_enc3_fold(Enc3Plan pl) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    for (uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); i < pl.p.nseg; i += nw) {
        const uint64_t b0 = ((gquad_ptr)pl.p.pbase)[i];
        bool comp;
        const uint64_t len = enc3_len(pl, i, &comp);
        const uint32_t m = (uint32_t)((len + kPiece - 1) >> kPieceLog);
        const uint32_t acc = m ? fold_part((gword_ptr)pl.p.praw + b0, m, lane) : 0u;
        const uint32_t crc = finish(acc, len);
        if (lane == 0) {
            ((gword_out)pl.p.crcs)[i] = crc;
            ((gword_out)pl.lens)[i] = (uint32_t)(len + PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE);
            ((gbyte_out)pl.kinds)[i] = comp ? PBSGPU_BLOB_ENCRYPTED_COMPRESSED : PBSGPU_BLOB_ENCRYPTED;
        }
        store_header(pl.p.dst + ((gquad_ptr)pl.p.doff)[i], lane, comp ? pl.zmagic_lo : pl.p.magic_lo,
                     comp ? pl.zmagic_hi : pl.p.magic_hi, crc);
    }
}

// the first min(len, 12) bytes of every blob (verify_device: the host parses the headers)
__global__ __launch_bounds__(256) void k_blob_heads(const uint8_t *src, const pbsgpu_segment *blobs, uint32_t n,
                                                    uint8_t *heads) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n * PBSGPU_BLOB_HEADER_SIZE) return;
    const uint32_t i = (uint32_t)(t / PBSGPU_BLOB_HEADER_SIZE), j = (uint32_t)(t % PBSGPU_BLOB_HEADER_SIZE);
    const pbsgpu_segment b{((gquad_ptr)blobs)[2 * i], ((gquad_ptr)blobs)[2 * i + 1]};
    ((gbyte_out)heads)[t] = j < b.length ? ((gbyte_ptr)src)[b.offset + j] : 0;
}

// ---- sources in up to two parts: the chunks of a page ring (pbsgpu_ring_blob_encode_device) ----------
// A ring chunk lies in one page or straddles two that are not neighbours in the arena. Every PART is a segment of its
// own for the piece pass (pieces aligned at the part's end, only its first piece short); a part knows how many of its
// leading bytes are among the chunk's first four (`inv`: a first part of 1-3 bytes leaves the rest to the second part).
// The fold joins the two parts with one more product: raw(A || B) = raw(A) * x^(8|B|) + raw(B), the constant from the
// host plan. The pair has kernels and a plan of its own; the walk is piece_raw with the unconditional store.
struct PartDesc {
    uint64_t src;    // offset of the part's first byte from PartPlan::base
    uint64_t dst;    // offset of where its bytes go in PartPlan::dst (behind the blob's header)
    uint32_t len;    // <= a page: < 2^31
    uint32_t inv;    // leading bytes that enter the CRC inverted (0..4)
    uint32_t pbase;  // index of its first piece
    uint32_t blob;   // the blob it belongs to (only the plan built on the device fills it in, for k_upz_pieces)
};
struct BlobDesc {
    uint64_t hdr;     // offset of the blob (its header) in PartPlan::dst
    uint32_t part0;   // its first part
    uint32_t nparts;  // 0 (empty chunk), 1 or 2
    uint32_t join;    // x^(8 |second part|)
    uint32_t len;     // data bytes
};
struct PartPlan {
    const uint8_t *base;
    const PartDesc *parts;
    const BlobDesc *blobs;   // nblob (nullptr for a plain copy)
    const uint32_t *ppart;   // npieces: part of each piece
    uint32_t *praw;          // npieces: raw CRC of each piece
    uint32_t *crcs;          // nblob
    uint8_t *dst;
    uint32_t npieces, nparts, nblob;
    uint32_t magic_lo, magic_hi;
    const uint32_t *counts;  // nullptr (the host-built plan: the three counts above), or npieces / nparts / nblob in device
                             // memory, from the plan kernels below: the launch grids then only know upper bounds
};
typedef const CRC_GLOBAL PartDesc *gpart_ptr;
typedef const CRC_GLOBAL BlobDesc *gblob_ptr;

// piece q of a range of len bytes whose first pinv bytes enter the CRC inverted: range bytes [lo, hi), inv of them inverted
struct PieceRange {
    uint32_t lo, hi, inv;
};
__device__ __forceinline__ PieceRange range_piece(uint32_t len, uint32_t pinv, uint32_t q) {
    const uint32_t m = (len + (uint32_t)kPiece - 1) >> kPieceLog;
    PieceRange r;
    r.hi = len - (m - 1 - q) * (uint32_t)kPiece;
    r.lo = r.hi > kPiece ? r.hi - (uint32_t)kPiece : 0;
    r.inv = r.lo < pinv ? (r.hi < pinv ? r.hi : pinv) - r.lo : 0u;
    return r;
}

__global__ __launch_bounds__(256) void k_pagecrc_pieces(PartPlan pl) {
    __shared__ uint32_t tab[17][256];
    build_tables(tab);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    const uint32_t npieces = pl.counts ? __builtin_amdgcn_readfirstlane(((gword_ptr)pl.counts)[0]) : pl.npieces;
    for (uint32_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); p < npieces; p += nw) {
        const uint32_t i = ((gword_ptr)pl.ppart)[p];
        const gpart_ptr pd = (gpart_ptr)pl.parts + i;
        const PieceRange r = range_piece(pd->len, pd->inv, p - pd->pbase);
        const uint32_t v = piece_raw(tab, pl.base + pd->src + r.lo, r.hi - r.lo, r.inv, lane, PutAll{pl.dst + pd->dst + r.lo});
        if (lane == 0) ((gword_out)pl.praw)[p] = v;
    }
}

// raw CRC of a blob's data from the pieces of its parts; the part boundary is a join whose shift is no power of two of kPiece
__device__ __forceinline__ uint32_t fold_blob(gword_ptr praw, gblob_ptr bd, gpart_ptr pd, uint32_t lane) {
    const uint32_t np = bd->nparts;
    uint32_t acc = 0;
    if (np >= 1) acc = fold_part(praw + pd[0].pbase, (pd[0].len + (uint32_t)kPiece - 1) >> kPieceLog, lane);
    if (np == 2) acc = mul(acc, bd->join) ^ fold_part(praw + pd[1].pbase, (pd[1].len + (uint32_t)kPiece - 1) >> kPieceLog, lane);
    return acc;
}

__global__ __launch_bounds__(256) void k_pagecrc_fold(PartPlan pl) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    const uint32_t nblob = pl.counts ? __builtin_amdgcn_readfirstlane(((gword_ptr)pl.counts)[2]) : pl.nblob;
    for (uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); i < nblob; i += nw) {
        const gblob_ptr bd = (gblob_ptr)pl.blobs + i;
        const uint32_t crc = finish(fold_blob((gword_ptr)pl.praw, bd, (gpart_ptr)pl.parts + bd->part0, lane), bd->len);
        if (lane == 0) ((gword_out)pl.crcs)[i] = crc;
        store_header(pl.dst + bd->hdr, lane, pl.magic_lo, pl.magic_hi, crc);
    }
}

// The same pair behind the encoder's verdict (pbsgpu_*_upload_new2_device with PBSGPU_ENCODE_F_ZSTD): what
// k_enc2_* are to k_crc_*. zstd_encode.hip has left res[blob] = frame length | kind << 56 and the frames that won behind
// their blobs' headers. A blob's pieces were planned for its slot, part by part; when its frame won they are numbered
// through as the pieces of ONE range, the frame where it lies (no store; it is shorter than the chunk, so the pieces past
// its end do nothing); otherwise they are the parts' pieces and the walk copies the chunk, as above.
struct UpzPlan {
    PartPlan p;
    const uint64_t *res;  // per blob
    uint32_t *lens;       // per blob: the blob's length
    uint8_t *kinds;       // per blob
    uint32_t zmagic_lo, zmagic_hi;  // the compressed kind's magic
};

__global__ __launch_bounds__(256) void k_upz_pieces(UpzPlan pl) {
    __shared__ uint32_t tab[17][256];
    build_tables(tab);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    const uint32_t npieces = __builtin_amdgcn_readfirstlane(((gword_ptr)pl.p.counts)[0]);
    for (uint32_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); p < npieces; p += nw) {
        const gpart_ptr pd = (gpart_ptr)pl.p.parts + ((gword_ptr)pl.p.ppart)[p];
        const uint32_t b = pd->blob;
        const uint64_t res = ((gquad_ptr)pl.res)[b];
        const uint8_t *from = pl.p.base + pd->src;
        uint8_t *o = pl.p.dst + pd->dst;
        uint32_t len = pd->len, pinv = pd->inv, q = p - pd->pbase;
        if ((res >> 56) == PBSGPU_BLOB_COMPRESSED) {  // (wave-uniform)
            const gblob_ptr bd = (gblob_ptr)pl.p.blobs + b;
            len = (uint32_t)res;  // below the chunk's length
            pinv = len < 4 ? 0u : 4u;
            q = p - ((gpart_ptr)pl.p.parts)[bd->part0].pbase;
            if (q >= (len + (uint32_t)kPiece - 1) >> kPieceLog) continue;
            from = pl.p.dst + bd->hdr + PBSGPU_BLOB_HEADER_SIZE;
            o = nullptr;
        }
        const PieceRange r = range_piece(len, pinv, q);
        const uint32_t v = piece_raw(tab, from + r.lo, r.hi - r.lo, r.inv, lane, PutIf{o ? o + r.lo : nullptr});
        if (lane == 0) ((gword_out)pl.p.praw)[p] = v;
    }
}

__global__ __launch_bounds__(256) void k_upz_fold(UpzPlan pl) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    const uint32_t nblob = __builtin_amdgcn_readfirstlane(((gword_ptr)pl.p.counts)[2]);
    for (uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); i < nblob; i += nw) {
        const gblob_ptr bd = (gblob_ptr)pl.p.blobs + i;
        const gpart_ptr pd = (gpart_ptr)pl.p.parts + bd->part0;
        const uint64_t res = ((gquad_ptr)pl.res)[i];
        const bool comp = (res >> 56) == PBSGPU_BLOB_COMPRESSED;
        const uint32_t len = comp ? (uint32_t)res : bd->len;
        const uint32_t acc = comp ? fold_part((gword_ptr)pl.p.praw + pd->pbase, (len + (uint32_t)kPiece - 1) >> kPieceLog, lane)
                                  : fold_blob((gword_ptr)pl.p.praw, bd, pd, lane);
        const uint32_t crc = finish(acc, len);
        if (lane == 0) {
            ((gword_out)pl.p.crcs)[i] = crc;
            ((gword_out)pl.lens)[i] = len + PBSGPU_BLOB_HEADER_SIZE;
            ((gbyte_out)pl.kinds)[i] = comp ? PBSGPU_BLOB_COMPRESSED : PBSGPU_BLOB_UNCOMPRESSED;
        }
        store_header(pl.p.dst + bd->hdr, lane, comp ? pl.zmagic_lo : pl.p.magic_lo, comp ? pl.zmagic_hi : pl.p.magic_hi, crc);
    }
}

// len bytes from d to o in 16-byte units plus a byte tail, by the workgroups that share blockIdx.y
__device__ __forceinline__ void copy_bytes(const uint8_t *d, uint8_t *o, uint32_t len) {
    const uint32_t units = len >> 4;
    const uint32_t sd = (uint32_t)(uintptr_t)d & 3u, so = (uint32_t)(uintptr_t)o & 3u;
    for (uint32_t u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
        uint32_t w[4];
        load16(d + 16ull * u, sd, w);
        store16(o + 16ull * u, so, w);
    }
    const uint32_t t = 16 * units + threadIdx.x;
    if (blockIdx.x == 0 && t < len) ((gbyte_out)o)[t] = ((gbyte_ptr)d)[t];
}

// the parts' bytes, unframed (pbsgpu_ring_copy_device): blockIdx.y strides over the parts, x over a part's 16-byte units
__global__ __launch_bounds__(256) void k_page_copy(PartPlan pl) {
    for (uint32_t i = blockIdx.y; i < pl.nparts; i += gridDim.y) {
        const gpart_ptr pd = (gpart_ptr)pl.parts + i;
        copy_bytes(pl.base + pd->src, pl.dst + pd->dst, pd->len);
    }
}


// ---- the plan built on the device: classify and frame in one call (pbsgpu_*_upload_new_device) --------
// Which records are new is known only on the device (the flags of k_known_mark), so what blob_encode_parts builds on the
// host is built here: per record its blob bytes, parts and pieces; exclusive prefix sums of the three (and of the blob
// count) give every descriptor its place. Three kernels over blocks of 256 records: the blocks' sums, one workgroup that
// scans those sums and decides whether the blobs fit, and the fill that repeats the per-record shape, scans inside its
// block and writes the descriptors. A fourth gives every piece its part.
struct UpCount {
    uint64_t bytes;  // 12 + size per new record
    uint32_t parts, pieces, blobs;
    uint32_t pad;
};
// (UpHead, the first 64 bytes of the block that goes back to the host: blob_plan.h)
struct UpPlan {
    const uint8_t *recs;           // n records (stride 48)
    const uint8_t *known;          // n: k_known_mark's flags
    const pbsgpu_segment *chunks;  // the contiguous form: chunk i is one part at chunks[i].offset (nullptr: the ring's pages)
    const PageTab *tabs;           // per stream slot: its logical pages [k0, k0 + n) are ptab[off ..)
    const uint64_t *ptab;          // offset of a page's body from PartPlan::base
    uint64_t page_bytes;
    uint64_t dst_cap;
    uint32_t stream;               // or PBSGPU_RING_ANY_STREAM: a record's stream is the low 28 bits of its segment
    uint32_t n;
    UpCount *bsum;                 // per block of 256 records: its sum, then (k_upnew_scan) the sum of the blocks before it
    UpHead *head;
    uint64_t *boff;                // n: blob offset of every new record
    uint8_t *skip;                 // n: the insert's flags (known, or all 1 when the blobs do not fit)
    PartDesc *parts;
    BlobDesc *blobs;
    uint32_t *ppart;
    zenc::Job *jobs;               // n, or nullptr: the encoder's jobs, of which the host knows the lengths and the blocks
};
typedef const CRC_GLOBAL UpCount *gcount_ptr;
typedef CRC_GLOBAL UpCount *gcount_out;
typedef const CRC_GLOBAL UpHead *ghead_ptr;

// a new record's bytes: part a at src0 and, when it straddles two pages, part b at src1
struct UpShape {
    uint64_t src0, src1;
    uint32_t a, b;
};
__device__ __forceinline__ bool up_shape(const UpPlan &pl, uint32_t i, UpShape &sh) {
    sh = UpShape{0, 0, 0, 0};
    if (i >= pl.n || ((gbyte_ptr)pl.known)[i]) return false;
    if (pl.chunks) {
        sh.src0 = ((gquad_ptr)pl.chunks)[2 * (uint64_t)i];
        sh.a = (uint32_t)((gquad_ptr)pl.chunks)[2 * (uint64_t)i + 1];
        return true;
    }
    const uint8_t *rc = pl.recs + 48ull * i;
    const uint32_t size = ((gword_ptr)rc)[11];
    if (size == 0) return true;
    const uint32_t sid = pl.stream == PBSGPU_RING_ANY_STREAM ? ((gword_ptr)rc)[10] & 0x0fffffffu : pl.stream;
    const uint64_t start = ((gquad_ptr)rc)[0] - size;
    const uint64_t k = start / pl.page_bytes, in = start - k * pl.page_bytes;
    const gquad_ptr tab = (gquad_ptr)pl.tabs + 2 * (uint64_t)sid;  // PageTab: k0 | off, n
    const gquad_ptr pg = (gquad_ptr)pl.ptab + (uint32_t)tab[1] + (k - tab[0]);
    sh.a = (uint32_t)(pl.page_bytes - in < size ? pl.page_bytes - in : size);
    sh.b = size - sh.a;
    sh.src0 = pg[0] + in;
    if (sh.b) sh.src1 = pg[1];
    return true;
}
__device__ __forceinline__ uint32_t up_pieces(uint32_t len) { return (len + (uint32_t)kPiece - 1) >> kPieceLog; }
__device__ __forceinline__ UpCount up_count(bool is_new, const UpShape &sh) {
    UpCount c{0, 0, 0, 0, 0};
    if (is_new) {
        c.bytes = (uint64_t)sh.a + sh.b + PBSGPU_BLOB_HEADER_SIZE;
        c.parts = (sh.a ? 1u : 0u) + (sh.b ? 1u : 0u);
        c.pieces = up_pieces(sh.a) + up_pieces(sh.b);
        c.blobs = 1;
    }
    return c;
}
__device__ __forceinline__ UpCount up_add(UpCount x, const UpCount &y) {
    x.bytes += y.bytes;
    x.parts += y.parts;
    x.pieces += y.pieces;
    x.blobs += y.blobs;
    return x;
}
// inclusive scan over the workgroup's 256 threads (ws: four entries of LDS); *total = the workgroup's sum
__device__ __forceinline__ UpCount up_block_scan(UpCount v, UpCount (&ws)[4], UpCount *total) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        UpCount u;
        u.bytes = __shfl_up((unsigned long long)v.bytes, d, 64);
        u.parts = __shfl_up(v.parts, d, 64);
        u.pieces = __shfl_up(v.pieces, d, 64);
        u.blobs = __shfl_up(v.blobs, d, 64);
        if (lane >= (uint32_t)d) v = up_add(v, u);
    }
    if (lane == 63) ws[w] = v;
    __syncthreads();
    UpCount pre{0, 0, 0, 0, 0}, tot{0, 0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const UpCount t = ws[j];
        if (j < w) pre = up_add(pre, t);
        tot = up_add(tot, t);
    }
    __syncthreads();  // (ws may be written again)
    *total = tot;
    return up_add(v, pre);
}
__device__ __forceinline__ void up_store(gcount_out o, const UpCount &c) {
    o->bytes = c.bytes;
    o->parts = c.parts;
    o->pieces = c.pieces;
    o->blobs = c.blobs;
}

__global__ __launch_bounds__(256) void k_upnew_count(UpPlan pl) {
    __shared__ UpCount ws[4];
    UpShape sh;
    const bool is_new = up_shape(pl, blockIdx.x * 256 + threadIdx.x, sh);
    UpCount tot;
    (void)up_block_scan(up_count(is_new, sh), ws, &tot);
    if (threadIdx.x == 0) up_store((gcount_out)pl.bsum + blockIdx.x, tot);
}

// one workgroup: the blocks' sums become exclusive prefixes; the totals and the verdict go to the head
__global__ __launch_bounds__(256) void k_upnew_scan(UpPlan pl) {
    __shared__ UpCount ws[4];
    const uint32_t nb = (pl.n + 255) / 256;
    UpCount carry{0, 0, 0, 0, 0};
    for (uint32_t b0 = 0; b0 < nb; b0 += 256) {
        const uint32_t b = b0 + threadIdx.x;
        UpCount v{0, 0, 0, 0, 0};
        if (b < nb) {
            const gcount_ptr q = (gcount_ptr)pl.bsum + b;
            v.bytes = q->bytes;
            v.parts = q->parts;
            v.pieces = q->pieces;
            v.blobs = q->blobs;
        }
        UpCount tot;
        const UpCount inc = up_block_scan(v, ws, &tot);
        if (b < nb) {
            UpCount ex = up_add(carry, inc);
            ex.bytes -= v.bytes;
            ex.parts -= v.parts;
            ex.pieces -= v.pieces;
            ex.blobs -= v.blobs;
            up_store((gcount_out)pl.bsum + b, ex);
        }
        carry = up_add(carry, tot);
    }
    if (threadIdx.x == 0) {
        CRC_GLOBAL UpHead *h = (CRC_GLOBAL UpHead *)pl.head;
        const bool over = carry.bytes > pl.dst_cap;
        h->total = carry.bytes;
        h->npieces = over ? 0u : carry.pieces;
        h->nparts = over ? 0u : carry.parts;
        h->nblob = over ? 0u : carry.blobs;
        h->over = over ? 1u : 0u;
        h->pad = 0;
    }
}

__global__ __launch_bounds__(256) void k_upnew_fill(UpPlan pl) {
    __shared__ UpCount ws[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    UpShape sh;
    const bool is_new = up_shape(pl, i, sh);
    const UpCount c = up_count(is_new, sh);
    UpCount tot;
    UpCount ex = up_block_scan(c, ws, &tot);
    if (i >= pl.n) return;
    ((gbyte_out)pl.skip)[i] = ((ghead_ptr)pl.head)->over ? (uint8_t)1 : (uint8_t)(is_new ? 0 : 1);
    if (!is_new) return;
    const gcount_ptr bp = (gcount_ptr)pl.bsum + blockIdx.x;
    const uint64_t hdr = bp->bytes + ex.bytes - c.bytes;
    const uint32_t part0 = bp->parts + ex.parts - c.parts;
    const uint32_t piece0 = bp->pieces + ex.pieces - c.pieces;
    const uint32_t len = sh.a + sh.b;
    uint32_t join = kOne;  // x^(8 b)
    for (int j = 0; j < 32; ++j)
        if ((sh.b >> j) & 1u) join = mul(join, kDev.x8[j]);
    const uint32_t blob = bp->blobs + ex.blobs - c.blobs;
    CRC_GLOBAL BlobDesc *bd = (CRC_GLOBAL BlobDesc *)pl.blobs + blob;
    bd->hdr = hdr;
    bd->part0 = part0;
    bd->nparts = c.parts;
    bd->join = join;
    bd->len = len;
    ((CRC_GLOBAL uint64_t *)pl.boff)[i] = hdr;
    if (pl.jobs && !((ghead_ptr)pl.head)->over) {  // where the chunk lies and where its frame would go: the job is live
        CRC_GLOBAL zenc::Job *jb = (CRC_GLOBAL zenc::Job *)pl.jobs + i;
        jb->src_off = sh.src0;
        jb->src1_off = sh.src1;
        jb->dst_off = hdr + PBSGPU_BLOB_HEADER_SIZE;
        jb->a = sh.a;
        jb->out = blob;
    }
    CRC_GLOBAL PartDesc *pd = (CRC_GLOBAL PartDesc *)pl.parts + part0;
    if (sh.a) {
        pd->src = sh.src0;
        pd->dst = hdr + PBSGPU_BLOB_HEADER_SIZE;
        pd->len = sh.a;
        pd->inv = len >= 4 ? (sh.a < 4 ? sh.a : 4u) : 0u;
        pd->pbase = piece0;
        pd->blob = blob;
    }
    if (sh.b) {  // (a first part of 1-3 bytes leaves the rest of the chunk's first four to this one)
        pd[1].src = sh.src1;
        pd[1].dst = hdr + PBSGPU_BLOB_HEADER_SIZE + sh.a;
        pd[1].len = sh.b;
        pd[1].inv = (len >= 4 && sh.a < 4) ? (4 - sh.a < sh.b ? 4 - sh.a : sh.b) : 0u;
        pd[1].pbase = piece0 + up_pieces(sh.a);
        pd[1].blob = blob;
    }
}

// the part of each piece: one thread per piece, a binary search for the last part that begins at or before it
__global__ __launch_bounds__(256) void k_upnew_ppart(UpPlan pl) {
    const ghead_ptr h = (ghead_ptr)pl.head;
    const uint32_t npieces = h->npieces, nparts = h->nparts;
    const gpart_ptr parts = (gpart_ptr)pl.parts;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < npieces; p += (uint64_t)gridDim.x * 256) {
        uint32_t lo = 0, hi = nparts;  // parts[lo].pbase <= p < parts[hi].pbase
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (parts[mid].pbase <= p) lo = mid;
            else hi = mid;
        }
        ((gword_out)pl.ppart)[p] = lo;
    }
}

// ---- the read side: (index, blobs) -> stream bytes (pbsgpu_blob_decode_device) ------------------------
// The mirror image of the encode pass over the DISTINCT blobs that the index slice references: one read of a blob's data
// gives its CRC and puts the bytes at their place in the stream. What kind a blob is and where its data begins is known
// only on the device (the magic), and nothing is read back in the middle, so the host plans the pieces for the 12-byte
// header and the kernels take the data start from k_dec_heads: an encrypted kind (44 bytes) may leave the first planned
// piece empty, raw CRC 0, which the fold passes over like the zero padding in front of a short piece.
//   k_dec_heads   per blob: magic -> kind and header length (0 = unknown magic or a cut header), the stored CRC, and the
//                 range launch_sha256_segments hashes (empty unless the blob is uncompressed)
//   k_dec_pieces  piece_raw with the CLIPPED store: the blob's data goes to the part of dst that belongs to its
//                 primary entry, cut at range_start / range_end at byte granularity while the CRC covers every byte;
//                 stored only when the blob is uncompressed and its data length is the entry's size
//   k_dec_fold    k_crc_fold over the data length the magic gives
//   k_dec_copy    the other entries that reference a blob (dedup fan-out), clipped in the same way, blob -> dst
//   k_dec_status  per entry, in pbsgpu_blob_verify's order: magic, CRC, kind, size, digest
// (DecInfo, DecStore and DecEntry, which the host plan fills in: blob_plan.h)
struct DecPlan {
    const uint8_t *src;
    const pbsgpu_segment *blobs;  // nu distinct referenced blobs (header included)
    const uint64_t *pbase;        // nu + 1
    const uint32_t *pseg;         // npieces
    uint32_t *praw;               // npieces
    uint32_t *crcs;               // nu
    DecInfo *info;                // nu
    pbsgpu_segment *sha;          // nu: what is hashed
    const DecStore *prim;         // nu: the store fused into the piece pass (xlo == xhi: none)
    const DecStore *copies;       // ncopy
    const DecEntry *ents;         // nidx
    const uint8_t *recs;          // nidx records (stride 48): the digests (nullptr: not checked)
    const uint8_t *digs;          // nu * 32: SHA-256 of the uncompressed blobs' data
    uint8_t *status;              // nidx
    uint8_t *dst;
    uint64_t npieces;
    uint32_t nu, ncopy, nidx;
};
typedef const CRC_GLOBAL DecStore *gstore_ptr;

// little-endian words of the four magics (kMagic below; a static_assert there ties the two together)
__device__ constexpr uint32_t kDecMagic[4][2] = {{0x0738AB42u, 0xA17083BEu},
                                                 {0x4258B931u, 0x7FA3B66Fu},
                                                 {0xBE85677Bu, 0xF04C2D22u},
                                                 {0xBF1B59E6u, 0x0BD8BF0Bu}};

__global__ __launch_bounds__(256) void k_dec_heads(DecPlan pl) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= pl.nu) return;
    const uint64_t off = ((gquad_ptr)pl.blobs)[2 * (uint64_t)u], len = ((gquad_ptr)pl.blobs)[2 * (uint64_t)u + 1];
    uint32_t w[3] = {0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < PBSGPU_BLOB_HEADER_SIZE; ++j)
        if (j < len) w[j >> 2] |= (uint32_t)((gbyte_ptr)pl.src)[off + j] << (8 * (j & 3));
    uint32_t hk = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t hdr = k >= PBSGPU_BLOB_ENCRYPTED ? PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE : PBSGPU_BLOB_HEADER_SIZE;
        if (len >= hdr && w[0] == kDecMagic[k][0] && w[1] == kDecMagic[k][1]) hk = hdr | (k << 8);
    }
    CRC_GLOBAL DecInfo *in = (CRC_GLOBAL DecInfo *)pl.info + u;
    in->hk = hk;
    in->stored = w[2];
    const bool plain = hk == PBSGPU_BLOB_HEADER_SIZE;  // uncompressed, header whole
    CRC_GLOBAL uint64_t *sh = (CRC_GLOBAL uint64_t *)pl.sha + 2 * (uint64_t)u;
    sh[0] = plain ? off + PBSGPU_BLOB_HEADER_SIZE : off;
    sh[1] = plain ? len - PBSGPU_BLOB_HEADER_SIZE : 0;
}

// At most 6 waves per SIMD, although its 53 VGPRs would allow 8: with all 8 workgroups of a CU resident at once the 4 MiB
// restore without digests measured 2 % slower (the rate table)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 6))) void k_dec_pieces(DecPlan pl) {
    __shared__ uint32_t tab[17][256];
    build_tables(tab);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    for (uint64_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); p < pl.npieces; p += nw) {
        const uint32_t u = ((gword_ptr)pl.pseg)[p];
        const uint64_t b0 = ((gquad_ptr)pl.pbase)[u];
        const uint64_t m = ((gquad_ptr)pl.pbase)[u + 1] - b0;
        const uint32_t hk = ((gword_ptr)pl.info)[2 * (uint64_t)u];
        const uint32_t hdr = hk & 255u;
        const uint64_t boff = ((gquad_ptr)pl.blobs)[2 * (uint64_t)u], blen = ((gquad_ptr)pl.blobs)[2 * (uint64_t)u + 1];
        const uint64_t dlen = hdr ? blen - hdr : 0;       // data bytes
        const uint64_t back = (m - 1 - (p - b0)) * kPiece;  // data bytes behind the piece
        if (back >= dlen) {  // no data (BAD_MAGIC), or the piece the 44-byte header leaves empty
            if (lane == 0) ((gword_out)pl.praw)[p] = 0;
            continue;
        }
        const uint64_t hi = dlen - back;  // piece = data bytes [lo, hi)
        const uint64_t lo = hi > kPiece ? hi - kPiece : 0;
        // the store: the piece's bytes [a, b) (piece coordinates) belong to the primary entry's part of dst
        const gstore_ptr ps = (gstore_ptr)pl.prim + u;
        const uint64_t xlo = ps->xlo, xhi = ps->xhi;
        const uint64_t cl = xlo > lo ? xlo : lo, ch = xhi < hi ? xhi : hi;
        const bool put = hk == PBSGPU_BLOB_HEADER_SIZE && dlen == ps->size && cl < ch;
        const PutClip clip{put ? pl.dst + ps->dofs + lo : nullptr, put ? (int32_t)(cl - lo) : 0, put ? (int32_t)(ch - lo) : 0};
        const uint32_t inv = (dlen >= 4 && lo < 4) ? (uint32_t)((hi < 4 ? hi : 4) - lo) : 0u;
        const uint32_t v = piece_raw(tab, pl.src + boff + hdr + lo, (uint32_t)(hi - lo), inv, lane, clip);
        if (lane == 0) ((gword_out)pl.praw)[p] = v;
    }
}

__global__ __launch_bounds__(256) void k_dec_fold(DecPlan pl) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    for (uint32_t u = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); u < pl.nu; u += nw) {
        const uint64_t b0 = ((gquad_ptr)pl.pbase)[u];
        const uint32_t hdr = ((gword_ptr)pl.info)[2 * (uint64_t)u] & 255u;
        const uint64_t blen = ((gquad_ptr)pl.blobs)[2 * (uint64_t)u + 1];
        // (an empty first piece has raw CRC 0 and is every merge's left half: it adds nothing)
        const uint32_t m = (uint32_t)(((gquad_ptr)pl.pbase)[u + 1] - b0);
        const uint32_t acc = m ? fold_part((gword_ptr)pl.praw + b0, m, lane) : 0u;
        const uint32_t crc = finish(acc, hdr ? blen - hdr : 0);
        if (lane == 0) ((gword_out)pl.crcs)[u] = crc;
    }
}

// blockIdx.y strides over the copies, x over a copy's 16-byte units (the shape of k_page_copy)
__global__ __launch_bounds__(256) void k_dec_copy(DecPlan pl) {
    for (uint32_t i = blockIdx.y; i < pl.ncopy; i += gridDim.y) {
        const gstore_ptr cs = (gstore_ptr)pl.copies + i;
        const uint32_t u = cs->u;
        const uint64_t boff = ((gquad_ptr)pl.blobs)[2 * (uint64_t)u], blen = ((gquad_ptr)pl.blobs)[2 * (uint64_t)u + 1];
        if (((gword_ptr)pl.info)[2 * (uint64_t)u] != PBSGPU_BLOB_HEADER_SIZE || blen - PBSGPU_BLOB_HEADER_SIZE != cs->size)
            continue;
        const uint64_t xlo = cs->xlo;
        copy_bytes(pl.src + boff + PBSGPU_BLOB_HEADER_SIZE + xlo, pl.dst + cs->dofs + xlo, (uint32_t)(cs->xhi - xlo));
    }
}

__global__ __launch_bounds__(256) void k_dec_status(DecPlan pl) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pl.nidx) return;
    const uint32_t u = ((gword_ptr)pl.ents)[2 * (uint64_t)i], size = ((gword_ptr)pl.ents)[2 * (uint64_t)i + 1];
    const uint32_t hk = ((gword_ptr)pl.info)[2 * (uint64_t)u], stored = ((gword_ptr)pl.info)[2 * (uint64_t)u + 1];
    const uint32_t hdr = hk & 255u;
    uint8_t r;
    if (hdr == 0) {
        r = PBSGPU_BLOB_BAD_MAGIC;
    } else if (((gword_ptr)pl.crcs)[u] != stored) {
        r = PBSGPU_BLOB_BAD_CRC;
    } else if (hk != PBSGPU_BLOB_HEADER_SIZE) {
        r = PBSGPU_BLOB_CRC_ONLY;
    } else if (((gquad_ptr)pl.blobs)[2 * (uint64_t)u + 1] - hdr != size) {
        r = PBSGPU_BLOB_BAD_SIZE;
    } else {
        r = PBSGPU_BLOB_OK;
        if (pl.recs) {
            const gword_ptr want = (gword_ptr)(pl.recs + 48ull * i + 8), got = (gword_ptr)(pl.digs + 32ull * u);
            uint32_t diff = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) diff |= want[j] ^ got[j];
            if (diff) r = PBSGPU_BLOB_BAD_DIGEST;
        }
    }
    ((gbyte_out)pl.status)[i] = r;
}

}  // namespace crc
}  // namespace pbsk

namespace {

using namespace pbsk::crc;
using namespace pbsp;

// SHA-256("Proxmox Backup ... blob v1.0")[0..8): uncompressed, zstd compressed, encrypted, zstd compressed encrypted
constexpr uint8_t kMagic[4][8] = {{66, 171, 56, 7, 190, 131, 112, 161},
                                  {49, 185, 88, 66, 111, 182, 163, 127},
                                  {123, 103, 133, 190, 34, 45, 76, 240},
                                  {230, 89, 27, 191, 11, 191, 216, 11}};

int magic_kind(const uint8_t *h) {
    for (int k = 0; k < 4; ++k)
        if (std::memcmp(h, kMagic[k], 8) == 0) return k;
    return -1;
}

uint64_t header_size(int kind) {
    return kind >= PBSGPU_BLOB_ENCRYPTED ? PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE : PBSGPU_BLOB_HEADER_SIZE;
}

uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the header's magic for the two encode plans: the uncompressed kind
template <class P>
void set_magic(P &pl) {
    pl.magic_lo = le32(kMagic[PBSGPU_BLOB_UNCOMPRESSED]);
    pl.magic_hi = le32(kMagic[PBSGPU_BLOB_UNCOMPRESSED] + 4);
}

// A piece kernel over np pieces (an upper bound when the plan's counts are on the device) and its fold over n ranges, on
// st. Waves stride over the work: 8 workgroups per CU for the pieces (17 KiB of tables each; every workgroup builds its
// tables once), 16 per CU for the fold.
template <class P>
int launch_pair(pbsgpu_engine *e, hipStream_t st, void (*pieces)(P), void (*fold)(P), const P &pl, uint64_t np, uint64_t n) {
    if (np) {
        const uint64_t wg = std::min<uint64_t>((np + 3) / 4, (uint64_t)e->num_cus * 8);
        hipLaunchKernelGGL(pieces, dim3((unsigned)wg), dim3(256), 0, st, pl);
        HIPCHK(hipGetLastError());
    }
    const uint64_t wg = std::min<uint64_t>((n + 3) / 4, (uint64_t)e->num_cus * 16);
    hipLaunchKernelGGL(fold, dim3((unsigned)wg), dim3(256), 0, st, pl);
    HIPCHK(hipGetLastError());
    return PBSGPU_OK;
}

// a plan's piece table onto the slot's scratch: pbase, pseg, and room for praw
int put_pieces(Slot *s, const PieceTable &t, Plan &pl) {
    CHK(put_table(s, t.pbase.data(), t.pbase.size(), &pl.pbase));
    CHK(put_table(s, t.owner.data(), t.owner.size(), &pl.pseg));
    pl.praw = s->take<uint32_t>((size_t)t.np);
    pl.npieces = t.np;
    return s->taken();
}

// CRC of the nseg ranges already in s->segs over device bytes d; optionally the encode destination. crcs_dev = the
// device result array (nseg u32). Enqueued on the slot's stream, nothing synchronised.
int enqueue_crc(pbsgpu_engine *e, Slot *s, const uint8_t *d, const pbsgpu_segment *segs, uint32_t nseg, uint8_t *dst,
                const uint64_t *offsets, uint32_t **crcs_dev) {
    PieceTable t;
    if (!piece_table(nseg, [&](uint64_t i) { return segs[i].length; }, t)) return PBSGPU_E_INVALID;
    Plan pl{};
    pl.src = d;
    pl.segs = s->segs.as<pbsgpu_segment>();
    pl.nseg = nseg;
    CHK(put_pieces(s, t, pl));
    pl.crcs = s->take<uint32_t>(nseg);
    CHK(s->taken());
    if (dst) {
        CHK(put_table(s, offsets, (size_t)nseg + 1, &pl.doff));
        pl.dst = dst;
        set_magic(pl);
    }
    CHK(launch_pair(e, s->stream, k_crc_pieces, k_crc_fold, pl, t.np, nseg));
    *crcs_dev = pl.crcs;
    return PBSGPU_OK;
}

int crc32_many(pbsgpu_engine *e, const void *ptr, bool host, uint64_t nbytes, const pbsgpu_segment *segs, uint32_t nseg,
               uint32_t *out) {
    if (!e || (!ptr && nbytes) || (nseg && (!segs || !out))) return PBSGPU_E_INVALID;
    if (!ranges_ok(segs, nseg, nbytes)) return PBSGPU_E_INVALID;
    if (nseg == 0) return PBSGPU_OK;
    if (!host && nbytes && !is_device_pointer(ptr)) return PBSGPU_E_INVALID;
    CHK(set_device(e));
    AuxLease lease(e);
    Slot *s = lease.s;
    const uint8_t *d = nullptr;
    CHK(stage_ranges(e, s, ptr, host, nbytes, segs, nseg, &d));
    uint32_t *crcs = nullptr;
    CHK(enqueue_crc(e, s, d, segs, nseg, nullptr, nullptr, &crcs));
    return fetch_result(s, out, crcs, (size_t)nseg * 4);
}

int encoded_size(const pbsgpu_segment *segs, uint32_t nseg, uint64_t *nbytes, uint64_t *offsets) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < nseg; ++i) {
        if (offsets) offsets[i] = total;
        const uint64_t b = segs[i].length + PBSGPU_BLOB_HEADER_SIZE;
        if (b < segs[i].length || total + b < total) return PBSGPU_E_INVALID;
        total += b;
    }
    if (offsets) offsets[nseg] = total;
    *nbytes = total;
    return PBSGPU_OK;
}

// pbsgpu_blob_encode2_device with PBSGPU_ENCODE_F_ZSTD: the frames (zstd_encode.hip), then the CRC pair over what each
// slot ended up holding, all on the slot's stream; one read-back of crcs, lens and kinds at the end.
int blob_encode_zstd(pbsgpu_engine *e, const uint8_t *src, const pbsgpu_segment *segs, uint32_t nseg, uint8_t *dst,
                     const uint64_t *offs, uint64_t src_bytes, uint32_t *lens, uint8_t *kinds, uint32_t *crcs) {
    AuxLease lease(e);
    Slot *s = lease.s;
    const uint8_t *d = nullptr;
    CHK(stage_ranges(e, s, src, false, src_bytes, segs, nseg, &d));
    std::vector<pbsk::zenc::Job> jobs(nseg);
    for (uint32_t i = 0; i < nseg; ++i)
        jobs[i] = pbsk::zenc::Job{segs[i].offset, 0, offs[i] + PBSGPU_BLOB_HEADER_SIZE, segs[i].length, (uint32_t)segs[i].length, 0, 0, 0};
    uint64_t *res = nullptr;
    CHK(pbsk::zenc::enqueue(e, s, d, dst, jobs, true, &res));
    PieceTable t;  // for each slot's capacity
    if (!piece_table(nseg, [&](uint64_t i) { return segs[i].length; }, t)) return PBSGPU_E_INVALID;
    const Enc2Block ob(nseg);  // crcs, lens, kinds: one block, read back once
    Enc2Plan pl{};
    pl.p.src = d;
    pl.p.segs = s->segs.as<pbsgpu_segment>();
    pl.p.nseg = nseg;
    CHK(put_pieces(s, t, pl.p));
    CHK(put_table(s, offs, (size_t)nseg + 1, &pl.p.doff));
    uint8_t *out = s->take<uint8_t>(ob.total);
    CHK(s->taken());
    pl.p.crcs = reinterpret_cast<uint32_t *>(out + ob.crcs);
    pl.p.dst = dst;
    set_magic(pl.p);
    pl.res = res;
    pl.lens = reinterpret_cast<uint32_t *>(out + ob.lens);
    pl.kinds = out + ob.kinds;
    pl.zmagic_lo = le32(kMagic[PBSGPU_BLOB_COMPRESSED]);
    pl.zmagic_hi = le32(kMagic[PBSGPU_BLOB_COMPRESSED] + 4);
    CHK(launch_pair(e, s->stream, k_enc2_pieces, k_enc2_fold, pl, t.np, nseg));
    std::vector<uint8_t> back(ob.total);
    CHK(fetch_result(s, back.data(), out, ob.total));  // the call's one synchronisation
    std::memcpy(crcs, back.data() + ob.crcs, (size_t)nseg * 4);
    std::memcpy(lens, back.data() + ob.lens, (size_t)nseg * 4);
    std::memcpy(kinds, back.data() + ob.kinds, nseg);
    return PBSGPU_OK;
}

// pbsgpu_blob_encode3_device with PBSGPU_ENCODE_F_AES: with zstd the frames at their blobs' data positions (byte 44), then
// the AES leg (aes_encode.hip: IV, ciphertext, tag), then the CRC pair over the ciphertexts where they lie, all on the
// slot's stream; one read-back of crcs, lens and kinds at the end. One piece table, for the slots' capacities, serves the
// cipher and the CRC.
int blob_encode_aes(pbsgpu_engine *e, const pbsgpu_aes_key *key, const uint8_t *ivs, bool zstd, const uint8_t *src,
                    const pbsgpu_segment *segs, uint32_t nseg, uint8_t *dst, const uint64_t *offs, uint64_t src_bytes,
                    uint32_t *lens, uint8_t *kinds, uint32_t *crcs) {
    AuxLease lease(e);
    Slot *s = lease.s;
    const uint8_t *d = nullptr;
    CHK(stage_ranges(e, s, src, false, src_bytes, segs, nseg, &d));
    uint64_t *res = nullptr;
    if (zstd) {
        std::vector<pbsk::zenc::Job> jobs(nseg);
        for (uint32_t i = 0; i < nseg; ++i)
            jobs[i] = pbsk::zenc::Job{segs[i].offset, 0, offs[i] + PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE, segs[i].length,
                                      (uint32_t)segs[i].length, 0, 0, 0};
        CHK(pbsk::zenc::enqueue(e, s, d, dst, jobs, true, &res));
    }
    PieceTable t;
    if (!capacity_pieces(segs, nseg, t)) return PBSGPU_E_INVALID;
    const Enc3Block ob(nseg);
    Enc3Plan pl{};
    pl.p.src = d;
    pl.p.segs = s->segs.as<pbsgpu_segment>();
    pl.p.nseg = nseg;
    CHK(put_pieces(s, t, pl.p));
    CHK(put_table(s, offs, (size_t)nseg + 1, &pl.p.doff));
    uint8_t *out = s->take<uint8_t>(ob.total);
    CHK(s->taken());
    pl.p.crcs = reinterpret_cast<uint32_t *>(out + ob.crcs);
    pl.p.dst = dst;
    pl.p.magic_lo = le32(kMagic[PBSGPU_BLOB_ENCRYPTED]);
    pl.p.magic_hi = le32(kMagic[PBSGPU_BLOB_ENCRYPTED] + 4);
    pl.res = res;
    pl.lens = reinterpret_cast<uint32_t *>(out + ob.lens);
    pl.kinds = out + ob.kinds;
    pl.zmagic_lo = le32(kMagic[PBSGPU_BLOB_ENCRYPTED_COMPRESSED]);
    pl.zmagic_hi = le32(kMagic[PBSGPU_BLOB_ENCRYPTED_COMPRESSED] + 4);
    const pbsk::aese::Job job{d, dst, pl.p.segs, pl.p.doff, res, pl.p.pbase, pl.p.pseg, nseg, (uint32_t)t.np};
    CHK(pbsk::aese::enqueue(e, s, key, job, ivs));
    CHK(launch_pair(e, s->stream, k_enc3_pieces, k_enc3_fold, pl, t.np, nseg));
    std::vector<uint8_t> back(ob.total);
    CHK(fetch_result(s, back.data(), out, ob.total));  // the call's one synchronisation
    std::memcpy(crcs, back.data() + ob.crcs, (size_t)nseg * 4);
    std::memcpy(lens, back.data() + ob.lens, (size_t)nseg * 4);
    std::memcpy(kinds, back.data() + ob.kinds, nseg);
    return PBSGPU_OK;
}

// the first PBSGPU_BLOB_HEADER_SIZE bytes of every blob (zero-padded when it is shorter) to the host
int read_heads(pbsgpu_engine *e, Slot *s, const void *ptr, bool host, uint64_t nbytes, const pbsgpu_segment *blobs, uint32_t n,
               std::vector<uint8_t> &heads) {
    heads.resize((size_t)n * PBSGPU_BLOB_HEADER_SIZE);
    if (host) {
        const uint8_t *h = static_cast<const uint8_t *>(ptr);
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = 0; j < PBSGPU_BLOB_HEADER_SIZE; ++j)
                heads[(size_t)i * PBSGPU_BLOB_HEADER_SIZE + j] = j < blobs[i].length ? h[blobs[i].offset + j] : 0;
        return PBSGPU_OK;
    }
    const uint8_t *d = nullptr;
    CHK(stage_ranges(e, s, ptr, false, nbytes, blobs, n, &d));
    uint8_t *heads_dev = s->take<uint8_t>(heads.size());
    CHK(s->taken());
    const uint64_t threads = heads.size();
    hipLaunchKernelGGL(pbsk::crc::k_blob_heads, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s->stream, d,
                       s->segs.as<pbsgpu_segment>(), n, heads_dev);
    HIPCHK(hipGetLastError());
    return fetch_result(s, heads.data(), heads_dev, heads.size());  // (synchronises: the staged ranges are free)
}

int blob_verify(pbsgpu_engine *e, const void *ptr, bool host, uint64_t nbytes, const pbsgpu_segment *blobs, uint32_t n,
                const uint8_t *digests, const uint32_t *sizes, uint8_t *status, pbsgpu_blob_stats *stats) {
    if (!e || (!ptr && nbytes) || (n && (!blobs || !status))) return PBSGPU_E_INVALID;
    if (!ranges_ok(blobs, n, nbytes)) return PBSGPU_E_INVALID;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return PBSGPU_OK;
    if (!host && nbytes && !is_device_pointer(ptr)) return PBSGPU_E_INVALID;
    CHK(set_device(e));
    AuxLease lease(e);
    Slot *s = lease.s;
    // 1. the headers, on the host
    std::vector<uint8_t> heads;
    CHK(read_heads(e, s, ptr, host, nbytes, blobs, n, heads));
    // 2. data ranges of the blobs with a known magic and a whole header: uncompressed ones first (the SHA-256 batch is a
    // prefix of the CRC batch)
    std::vector<int> kind(n);
    std::vector<pbsgpu_segment> data;
    std::vector<uint32_t> which;
    data.reserve(n);
    which.reserve(n);
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t i = 0; i < n; ++i) {
            if (pass == 0) {
                const int k = blobs[i].length >= 8 ? magic_kind(&heads[(size_t)i * PBSGPU_BLOB_HEADER_SIZE]) : -1;
                kind[i] = (k >= 0 && blobs[i].length >= header_size(k)) ? k : -1;
            }
            if (kind[i] < 0 || (kind[i] == PBSGPU_BLOB_UNCOMPRESSED) != (pass == 0)) continue;
            const uint64_t hdr = header_size(kind[i]);
            data.push_back(pbsgpu_segment{blobs[i].offset + hdr, blobs[i].length - hdr});
            which.push_back(i);
        }
    uint32_t nunc = 0;
    while (nunc < which.size() && kind[which[nunc]] == PBSGPU_BLOB_UNCOMPRESSED) ++nunc;
    const uint32_t nd = (uint32_t)data.size();
    std::vector<uint32_t> crc(nd);
    std::vector<uint8_t> dig(digests ? (size_t)nunc * 32 : 0);
    if (nd) {
        const uint8_t *d = nullptr;
        CHK(stage_ranges(e, s, ptr, host, nbytes, data.data(), nd, &d));
        uint32_t *crcs = nullptr;
        CHK(enqueue_crc(e, s, d, data.data(), nd, nullptr, nullptr, &crcs));
        uint8_t *digs_dev = nullptr;
        if (digests && nunc) {
            ShaWork work;
            for (uint32_t j = 0; j < nunc; ++j) work.add(data[j].length);
            digs_dev = s->take<uint8_t>((size_t)nunc * 32);
            CHK(s->taken());
            CHK(enqueue_sha256(e, s->stream, d, s->segs.as<pbsgpu_segment>(), nunc, digs_dev,
                               s->scalars.as<uint32_t>() + SC_QUEUE, work));
        }
        CHK(fetch_result(s, crc.data(), crcs, (size_t)nd * 4));
        if (digs_dev) CHK(fetch_result(s, dig.data(), digs_dev, (size_t)nunc * 32));
    }
    // 3. the statuses, in the order of the checks
    pbsgpu_blob_stats st{};
    for (uint32_t i = 0; i < n; ++i) {
        status[i] = PBSGPU_BLOB_BAD_MAGIC;
        st.blob_bytes += blobs[i].length;
    }
    for (uint32_t j = 0; j < nd; ++j) {
        const uint32_t i = which[j];
        st.crc_bytes += data[j].length;
        uint8_t r;
        if (crc[j] != le32(&heads[(size_t)i * PBSGPU_BLOB_HEADER_SIZE + 8]))
            r = PBSGPU_BLOB_BAD_CRC;
        else if (kind[i] != PBSGPU_BLOB_UNCOMPRESSED)
            r = PBSGPU_BLOB_CRC_ONLY;
        else if (sizes && data[j].length != sizes[i])
            r = PBSGPU_BLOB_BAD_SIZE;
        else if (digests && std::memcmp(&dig[(size_t)j * 32], digests + (size_t)i * 32, 32) != 0)
            r = PBSGPU_BLOB_BAD_DIGEST;
        else
            r = PBSGPU_BLOB_OK;
        if (digests && j < nunc) st.sha_bytes += data[j].length;
        status[i] = r;
    }
    for (uint32_t i = 0; i < n; ++i) st.count[status[i]]++;
    if (stats) *stats = st;
    return PBSGPU_OK;
}

constexpr bool magic_words_match() {
    for (int k = 0; k < 4; ++k)
        for (int h = 0; h < 2; ++h) {
            uint32_t w = 0;
            for (int j = 0; j < 4; ++j) w |= (uint32_t)kMagic[k][4 * h + j] << (8 * j);
            if (w != kDecMagic[k][h]) return false;
        }
    return true;
}
static_assert(magic_words_match(), "kDecMagic is kMagic in little-endian words");

// pbsgpu_blob_decode*_device past "no engine" and "nothing to do": the argument checks, in their order
int check_decode(pbsgpu_engine *e, const void *bptr, uint64_t nbytes, const pbsgpu_segment *blobs, uint32_t nblob,
                 const pbsgpu_record *idx, uint64_t nidx, const uint32_t *blob_of, uint64_t rs, uint64_t re, bool zstd,
                 const void *dst, uint64_t dst_cap) {
    if (!idx || !blobs || nblob == 0 || (!bptr && nbytes)) return PBSGPU_E_INVALID;
    if (!blob_of && nblob != nidx) return PBSGPU_E_INVALID;
    if (!ranges_ok(blobs, nblob, nbytes)) return PBSGPU_E_INVALID;
    if (zstd)  // the frame decoder counts in 32 bits (a chunk is 16 MiB at the most)
        for (uint32_t b = 0; b < nblob; ++b)
            if (blobs[b].length >> 32) return PBSGPU_E_INVALID;
    for (uint64_t i = 0; i < nidx; ++i) {
        if (blob_of && blob_of[i] >= nblob) return PBSGPU_E_INVALID;
        if (idx[i].size > idx[i].end || (i && idx[i].end - idx[i].size != idx[i - 1].end)) return PBSGPU_E_INVALID;
    }
    const uint64_t S = idx[0].end - idx[0].size, E = idx[nidx - 1].end;
    if (rs < S || rs > re || re > E) return PBSGPU_E_INVALID;
    const uint64_t need = re - rs;
    if (need && (!dst || overlaps(dst, need, bptr, nbytes))) return PBSGPU_E_INVALID;  // dst overlaps the blob buffer
    CHK(set_device(e));
    if ((nbytes && !is_device_pointer(bptr)) || (need && !is_device_pointer(dst))) return PBSGPU_E_INVALID;
    return dst_cap < need ? PBSGPU_E_CAPACITY : PBSGPU_OK;
}

// The restore's own kernels on the slot's stream, nothing synchronised: the heads, the CRC pair with the primary stores
// fused in, the other entries' copies, the digests of the uncompressed blobs and the statuses. `out` is the block that
// goes back (DecBlock); pl is left filled in for the zstd leg.
int enqueue_restore(pbsgpu_engine *e, Slot *s, const Restore &r, const void *bptr, uint64_t nbytes, const pbsgpu_record *idx,
                    bool check_digest, uint8_t *dst, const DecBlock &ob, uint8_t **out, DecPlan &pl) {
    const uint32_t nu = r.nu();
    const size_t nidx = r.ents.size(), ncopy = r.copies.size();
    const DecTables tl(nu, ncopy, nidx, (size_t)r.pieces.np);
    std::vector<uint8_t> tabs(tl.total);
    const auto pack = [&](size_t at, const void *from, size_t bytes) {
        if (bytes) std::memcpy(tabs.data() + at, from, bytes);
    };
    pack(tl.pbase, r.pieces.pbase.data(), ((size_t)nu + 1) * 8);
    pack(tl.prim, r.prim.data(), (size_t)nu * sizeof(DecStore));
    pack(tl.copies, r.copies.data(), ncopy * sizeof(DecStore));
    pack(tl.ents, r.ents.data(), nidx * sizeof(DecEntry));
    pack(tl.pseg, r.pieces.owner.data(), (size_t)r.pieces.np * 4);
    pl = DecPlan{};
    CHK(stage_ranges(e, s, bptr, false, nbytes, r.ub.data(), nu, &pl.src));
    const uint8_t *t = nullptr;
    CHK(put_table(s, tabs.data(), tabs.size(), &t));
    pl.praw = s->take<uint32_t>((size_t)r.pieces.np);
    pl.crcs = s->take<uint32_t>(nu);
    pl.sha = s->take<pbsgpu_segment>(nu);
    *out = s->take<uint8_t>(ob.total);
    uint8_t *digs = check_digest ? s->take<uint8_t>((size_t)nu * 32) : nullptr;
    CHK(s->taken());
    if (check_digest) CHK(put_table(s, reinterpret_cast<const uint8_t *>(idx), nidx * sizeof(pbsgpu_record), &pl.recs));
    pl.blobs = s->segs.as<pbsgpu_segment>();
    pl.pbase = reinterpret_cast<const uint64_t *>(t + tl.pbase);
    pl.prim = reinterpret_cast<const DecStore *>(t + tl.prim);
    pl.copies = reinterpret_cast<const DecStore *>(t + tl.copies);
    pl.ents = reinterpret_cast<const DecEntry *>(t + tl.ents);
    pl.pseg = reinterpret_cast<const uint32_t *>(t + tl.pseg);
    pl.info = reinterpret_cast<DecInfo *>(*out + ob.info);
    pl.digs = digs;
    pl.status = *out + ob.status;
    pl.dst = dst;
    pl.npieces = r.pieces.np;
    pl.nu = nu;
    pl.ncopy = (uint32_t)ncopy;
    pl.nidx = (uint32_t)nidx;
    hipLaunchKernelGGL(pbsk::crc::k_dec_heads, dim3((nu + 255) / 256), dim3(256), 0, s->stream, pl);
    HIPCHK(hipGetLastError());
    CHK(launch_pair(e, s->stream, k_dec_pieces, k_dec_fold, pl, r.pieces.np, nu));
    if (pl.ncopy) {  // grid as for k_page_copy
        const uint32_t gx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((r.longest_copy / 16 + 255) / 256, (uint64_t)e->num_cus * 8));
        hipLaunchKernelGGL(pbsk::crc::k_dec_copy, dim3(gx, std::min<uint32_t>(pl.ncopy, 1024)), dim3(256), 0, s->stream, pl);
        HIPCHK(hipGetLastError());
    }
    if (check_digest)  // on the sizes the host knows (exact for uncompressed blobs)
        CHK(enqueue_sha256(e, s->stream, pl.src, pl.sha, nu, digs, s->scalars.as<uint32_t>() + SC_QUEUE, r.sha));
    hipLaunchKernelGGL(pbsk::crc::k_dec_status, dim3((unsigned)((nidx + 255) / 256)), dim3(256), 0, s->stream, pl);
    HIPCHK(hipGetLastError());
    return PBSGPU_OK;
}

// The zstd leg (zstd.hip), behind the statuses above on the same stream: the frames of the compressed blobs with a good
// CRC into the rooms the plan gave them, the copies out of scratch, the digests of the decoded bytes, and the statuses
// of the decoded blobs' entries. zres: the frames' results in the block that goes back.
// run = false: rooms, copies and scratch are laid out and *plan filled in for the AES leg, nothing of the zstd leg is launched.
int enqueue_restore_zstd(pbsgpu_engine *e, Slot *s, Restore &r, const DecPlan &pl, uint64_t *zres, bool run,
                         pbsk::zstd::RestorePlan *plan) {
    namespace pz = pbsk::zstd;
    const uint32_t nu = r.nu();
    uint8_t *scratch = s->bulk((size_t)r.scratch_bytes);
    CHK(s->taken());
    r.place_scratch((uint64_t)((uintptr_t)scratch - (uintptr_t)pl.dst));
    const ZTables zl(nu, r.zcopies.size());
    std::vector<uint8_t> ztab(zl.total);
    std::memcpy(ztab.data() + zl.jobs, r.jobs.data(), (size_t)nu * sizeof(pz::RestoreJob));
    if (!r.zcopies.empty()) std::memcpy(ztab.data() + zl.copies, r.zcopies.data(), r.zcopies.size() * sizeof(pz::RestoreCopy));
    const uint8_t *zt = nullptr;
    CHK(put_table(s, ztab.data(), ztab.size(), &zt));
    const ZWork zw(nu);
    uint8_t *w = s->take<uint8_t>(zw.total);
    CHK(s->taken());
    pz::RestorePlan zp{};
    zp.src = pl.src;
    zp.blobs = pl.blobs;
    zp.info = reinterpret_cast<const uint32_t *>(pl.info);
    zp.crcs = pl.crcs;
    zp.jobs = reinterpret_cast<const pz::RestoreJob *>(zt + zl.jobs);
    zp.copies = reinterpret_cast<const pz::RestoreCopy *>(zt + zl.copies);
    zp.ents = reinterpret_cast<const uint32_t *>(pl.ents);
    zp.recs = pl.recs;
    zp.digs = w + zw.digs;
    zp.res = zres;
    zp.sha = reinterpret_cast<pbsgpu_segment *>(w + zw.sha);
    zp.status = pl.status;
    zp.dst = pl.dst;
    zp.lit = scratch;
    zp.nu = nu;
    zp.ncopy = (uint32_t)r.zcopies.size();
    zp.nidx = pl.nidx;
    zp.stride = r.lit_groups;
    if (plan) *plan = zp;
    if (!run) return PBSGPU_OK;
    HIPCHK(pz::launch_restore_frames(zp, w + zw.desc, s->stream));
    if (zp.ncopy) HIPCHK(pz::launch_restore_copy(zp, r.longest_zcopy, e->num_cus, s->stream));
    if (pl.recs) {
        uint32_t *zq = reinterpret_cast<uint32_t *>(w + zw.queue);
        HIPCHK(hipMemsetAsync(zq, 0, 64, s->stream));
        CHK(enqueue_sha256(e, s->stream, zp.dst, zp.sha, nu, w + zw.digs, zq, r.zsha));
    }
    HIPCHK(pz::launch_restore_status(zp, s->stream));
    return PBSGPU_OK;
}

// the statistics of a restore from the block that came back
void restore_stats(const Restore &r, const uint8_t *back, const DecBlock &ob, bool check_digest, bool zstd, bool aes,
                   const uint8_t *status, pbsgpu_decode_stats3 *stats, bool keyed = false) {
    const uint32_t nu = r.nu();
    const size_t nidx = r.ents.size();
    const DecInfo *info = reinterpret_cast<const DecInfo *>(back + ob.info);
    for (uint32_t u = 0; u < nu; ++u) {
        const uint32_t hdr = info[u].hk & 255u;
        stats->blob_bytes += r.ub[u].length;
        if (hdr) stats->crc_bytes += r.ub[u].length - hdr;
        if (check_digest && info[u].hk == PBSGPU_BLOB_HEADER_SIZE) stats->sha_bytes += r.ub[u].length - hdr;
    }
    for (size_t i = 0; i < nidx; ++i) {
        stats->count[status[i]]++;
        const uint32_t u = r.ents[i].u;
        if (info[u].hk == PBSGPU_BLOB_HEADER_SIZE && r.ub[u].length - PBSGPU_BLOB_HEADER_SIZE == r.ents[i].size)
            stats->out_bytes += r.clip[i];
    }
    if (aes) {  // the AES leg's results: once per distinct blob it decrypted
        const uint64_t *ares = reinterpret_cast<const uint64_t *>(back + ob.ares);
        for (uint32_t u = 0; u < nu; ++u) {
            const uint32_t code = (uint32_t)(ares[u] >> 32);
            if (code == pbsk::zstd::kNotDecoded) continue;
            const uint64_t len = r.ub[u].length - PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE;
            stats->aes_bytes += len;
            // with the id key: the plaintext of every blob the leg restored was hashed once, keyed
            if (keyed && (code & ~pbsk::aes::kResFrame) == PBSGPU_ZSTD_OK) stats->sha_bytes += (uint32_t)ares[u];
            if (code == pbsk::aes::kResBadTag || !(code & pbsk::aes::kResFrame)) continue;
            stats->zstd_in_bytes += len;  // a good tag over a frame: it went to the decoder
            if (code == (pbsk::aes::kResFrame | PBSGPU_ZSTD_OK)) stats->zstd_out_bytes += (uint32_t)ares[u];
        }
        for (size_t i = 0; i < nidx; ++i) {
            const uint64_t a = ares[r.ents[i].u];
            if ((a & ~((uint64_t)pbsk::aes::kResFrame << 32)) == (uint64_t)r.ents[i].size) stats->out_bytes += r.clip[i];
        }
    }
    if (!zstd) return;
    const uint64_t *zres = reinterpret_cast<const uint64_t *>(back + ob.zres);
    for (uint32_t u = 0; u < nu; ++u) {
        if ((uint32_t)(zres[u] >> 32) == pbsk::zstd::kNotDecoded) continue;
        stats->zstd_in_bytes += r.ub[u].length - PBSGPU_BLOB_HEADER_SIZE;
        if ((zres[u] >> 32) != PBSGPU_ZSTD_OK) continue;
        stats->zstd_out_bytes += (uint32_t)zres[u];
        if (check_digest) stats->sha_bytes += (uint32_t)zres[u];
    }
    for (size_t i = 0; i < nidx; ++i)
        if (zres[r.ents[i].u] == (uint64_t)r.ents[i].size) stats->out_bytes += r.clip[i];  // status OK, the entry's size
}

// pbsgpu_blob_decode*_device: check, plan (blob_plan.h: everything the host can know is decided there, before any device
// work), enqueue, and the statistics from the one block that comes back. What depends on the blobs' bytes (kind, data
// length, CRC, digest, the frames) is decided on the device.
int blob_decode(pbsgpu_engine *e, const void *bptr, uint64_t nbytes, const pbsgpu_segment *blobs, uint32_t nblob,
                const pbsgpu_record *idx, uint64_t nidx, const uint32_t *blob_of, uint64_t rs, uint64_t re,
                uint32_t flags, const pbsgpu_aes_key *key, void *dst, uint64_t dst_cap, uint8_t *status,
                pbsgpu_decode_stats3 *stats, const pbsgpu_id_key *idkey = nullptr) {
    const bool check_digest = (flags & PBSGPU_DECODE_F_DIGEST) != 0;
    const bool zstd = (flags & PBSGPU_DECODE_F_ZSTD) != 0;
    const bool aes = (flags & PBSGPU_DECODE_F_AES) != 0;
    if (!e || nidx >= (1ull << 32)) return PBSGPU_E_INVALID;
    if (aes && (!key || pbsk::aes::key_engine(key) != e)) return PBSGPU_E_INVALID;
    if (idkey && idkey->eng != e) return PBSGPU_E_INVALID;
    const bool keyed = idkey && aes && check_digest;  // (an id key without F_AES or without F_DIGEST is ignored)
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (nidx == 0) return PBSGPU_OK;
    if (!status) return PBSGPU_E_INVALID;
    CHK(check_decode(e, bptr, nbytes, blobs, nblob, idx, nidx, blob_of, rs, re, zstd || aes, dst, dst_cap));
    Restore r;  // (the rooms and copies of a transformed blob are the same for either leg)
    if (!plan_restore(blobs, nblob, idx, nidx, blob_of, rs, re, zstd || aes, (uint64_t)e->num_cus * 4, r)) return PBSGPU_E_INVALID;
    AuxLease lease(e);
    Slot *s = lease.s;
    const DecBlock ob(r.nu(), (size_t)nidx, zstd, aes);
    uint8_t *out = nullptr;
    DecPlan pl;
    CHK(enqueue_restore(e, s, r, bptr, nbytes, idx, check_digest, static_cast<uint8_t *>(dst), ob, &out, pl));
    if (zstd || aes) {
        pbsk::zstd::RestorePlan zp{};
        CHK(enqueue_restore_zstd(e, s, r, pl, reinterpret_cast<uint64_t *>(out + ob.zres), zstd, &zp));
        if (aes)
            CHK(pbsk::aes::enqueue_restore(e, s, key, zp, r.ub.data(), zstd, r.longest_zcopy,
                                           reinterpret_cast<uint64_t *>(out + ob.ares), keyed ? idkey->dev() : nullptr, &r.zsha));
    }
    std::vector<uint8_t> back(ob.total);
    CHK(fetch_result(s, back.data(), out, ob.total));  // the call's one synchronisation
    std::memcpy(status, back.data() + ob.status, (size_t)nidx);
    if (stats) restore_stats(r, back.data(), ob, check_digest, zstd, aes, status, stats, keyed);
    return PBSGPU_OK;
}

}  // namespace

namespace pbse {

using namespace pbsk::crc;
using namespace pbsp;

// the plan's tables onto the aux slot and the launch pair (or the copy kernel) behind them; nothing synchronised
static int enqueue_parts(pbsgpu_engine *e, Slot *s, PartPlan &pl, const std::vector<PartDesc> &parts,
                         const std::vector<BlobDesc> &blobs, const std::vector<uint32_t> &ppart) {
    CHK(put_table(s, parts.data(), parts.size(), &pl.parts));
    pl.nparts = (uint32_t)parts.size();
    if (blobs.empty()) {
        uint32_t longest = 0;
        for (const PartDesc &p : parts) longest = std::max(longest, p.len);
        const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((longest / 16 + 255) / 256, (uint32_t)e->num_cus * 8));
        const uint32_t gy = std::min<uint32_t>(pl.nparts, 1024);
        hipLaunchKernelGGL(pbsk::crc::k_page_copy, dim3(gx, gy), dim3(256), 0, s->stream, pl);
        HIPCHK(hipGetLastError());
        return PBSGPU_OK;
    }
    CHK(put_table(s, blobs.data(), blobs.size(), &pl.blobs));
    CHK(put_table(s, ppart.data(), ppart.size(), &pl.ppart));
    pl.praw = s->take<uint32_t>(ppart.size());
    pl.crcs = s->take<uint32_t>(blobs.size());
    CHK(s->taken());
    pl.npieces = (uint32_t)ppart.size();
    pl.nblob = (uint32_t)blobs.size();
    set_magic(pl);
    return launch_pair(e, s->stream, k_pagecrc_pieces, k_pagecrc_fold, pl, pl.npieces, pl.nblob);
}

int blob_encode_parts(pbsgpu_engine *e, const uint8_t *base, const SrcPart (*src)[2], uint32_t nblob, uint8_t *dst,
                      const uint64_t *doff, uint32_t *crcs) {
    if (nblob == 0) return PBSGPU_OK;
    std::vector<PartDesc> parts;
    std::vector<BlobDesc> blobs(nblob);
    parts.reserve((size_t)nblob + nblob / 8 + 1);
    uint64_t np = 0;
    for (uint32_t i = 0; i < nblob; ++i) {
        const uint64_t len = (uint64_t)src[i][0].len + src[i][1].len;
        BlobDesc &b = blobs[i];
        b.hdr = doff[i];
        b.part0 = (uint32_t)parts.size();
        b.nparts = 0;
        b.len = (uint32_t)len;
        b.join = src[i][1].len ? pow_from(kHost.x8, src[i][1].len) : kOne;
        uint32_t done = 0;  // chunk bytes in front of the part
        for (int k = 0; k < 2; ++k) {
            const SrcPart &sp = src[i][k];
            if (sp.len == 0) continue;
            PartDesc p{};
            p.src = sp.src;
            p.dst = doff[i] + PBSGPU_BLOB_HEADER_SIZE + done;
            p.len = sp.len;
            p.inv = (len >= 4 && done < 4) ? std::min<uint32_t>(4 - done, sp.len) : 0u;
            p.pbase = (uint32_t)np;
            np += (sp.len + kPiece - 1) >> kPieceLog;
            done += sp.len;
            parts.push_back(p);
            b.nparts++;
        }
        if (len >= (1ull << 32) || np >= (1ull << 32) || parts.size() >= (1ull << 32)) return PBSGPU_E_INVALID;
    }
    std::vector<uint32_t> ppart((size_t)np);
    for (uint32_t j = 0; j < parts.size(); ++j) {
        const uint32_t end = j + 1 < parts.size() ? parts[j + 1].pbase : (uint32_t)np;
        for (uint32_t p = parts[j].pbase; p < end; ++p) ppart[p] = j;
    }
    CHK(set_device(e));
    AuxLease lease(e);
    Slot *s = lease.s;
    PartPlan pl{};
    pl.base = base;
    pl.dst = dst;
    CHK(enqueue_parts(e, s, pl, parts, blobs, ppart));
    if (crcs) return fetch_result(s, crcs, pl.crcs, (size_t)nblob * 4);
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBSGPU_OK;
}

int copy_parts(pbsgpu_engine *e, const uint8_t *base, const SrcPart *src, uint32_t nparts, uint8_t *dst) {
    std::vector<PartDesc> parts;
    uint64_t done = 0;
    for (uint32_t j = 0; j < nparts; ++j) {
        if (src[j].len == 0) continue;
        PartDesc p{};
        p.src = src[j].src;
        p.dst = done;
        p.len = src[j].len;
        done += src[j].len;
        parts.push_back(p);
    }
    if (parts.empty()) return PBSGPU_OK;
    CHK(set_device(e));
    AuxLease lease(e);
    Slot *s = lease.s;
    PartPlan pl{};
    pl.base = base;
    pl.dst = dst;
    CHK(enqueue_parts(e, s, pl, parts, {}, {}));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBSGPU_OK;
}

// what one upload_new call has on the device
struct UpDev {
    KnownPass p;
    UpPlan up{};
    pbsk::zenc::Room room{};
    uint32_t *praw = nullptr;
    uint8_t *out = nullptr;  // the block that goes back (UpBlock)
};

// The call's arrays from the slot's scratch, and the host's tables onto them: the small source table first (the PageTabs
// and the page array of the ring form, or the chunk ranges of the contiguous form), so that the records' copy waits for
// nothing but that; with F_ZSTD the encoder's room, its jobs staged with the lengths and blocks, none of them live
// (k_upnew_fill makes the new records' jobs live).
static int stage_upload(Slot *s, const UploadSrc &src, const pbsgpu_record *recs, uint64_t n, const UpBlock &ob,
                        const pbsk::zenc::Prep *zp, const std::vector<pbsk::zenc::Job> &jobs, UpDev &dv) {
    KnownPass &p = dv.p;
    UpPlan &up = dv.up;
    CHK(known_sort_bytes(n, s->stream, &p.tmp_bytes));
    if (src.chunks) {
        CHK(put_table(s, src.chunks, (size_t)n, &up.chunks));
    } else {
        const uint64_t *tabs = nullptr;
        CHK(put_table(s, src.tabs, src.tab_words, &tabs));
        up.tabs = reinterpret_cast<const PageTab *>(tabs);
        up.ptab = tabs + 2 * (size_t)src.nslots;
    }
    CHK(put_table(s, reinterpret_cast<const uint8_t *>(recs), (size_t)n * sizeof(pbsgpu_record), &p.recs));
    p.keys = s->take<uint32_t>((size_t)n * 2);  // sort keys and indices, each with its double buffer
    p.idx = s->take<uint32_t>((size_t)n * 2);
    p.before = s->take<uint8_t>((size_t)n * 2);  // before | skip
    p.tmp = s->take<uint8_t>(p.tmp_bytes);
    up.bsum = s->take<UpCount>((size_t)((n + 255) / 256));
    up.parts = s->take<PartDesc>((size_t)std::min<uint64_t>(2 * n, src.pieces_max));
    up.blobs = s->take<BlobDesc>((size_t)n);
    up.ppart = s->take<uint32_t>((size_t)src.pieces_max);
    dv.praw = s->take<uint32_t>((size_t)src.pieces_max);
    dv.out = s->take<uint8_t>(ob.total);
    CHK(s->taken());
    CHK(s->h_recs.ensure(ob.total + 64));
    CHK(s->h_scalars.ensure(64));
    if (zp) CHK(pbsk::zenc::carve(s, *zp, jobs, dv.room));
    p.stride = sizeof(pbsgpu_record);
    p.n = n;
    p.known = dv.out + ob.known;
    p.stats = reinterpret_cast<uint64_t *>(dv.out + ob.head);
    up.recs = p.recs;
    up.known = p.known;
    up.page_bytes = src.page_bytes;
    up.stream = src.stream;
    up.n = (uint32_t)n;
    up.head = reinterpret_cast<UpHead *>(dv.out + ob.head);
    up.boff = reinterpret_cast<uint64_t *>(dv.out + ob.boff);
    up.skip = p.before + n;
    up.jobs = dv.room.jobs;
    return PBSGPU_OK;
}

// the plan kernels: per record its blob, parts and pieces, and the verdict whether the blobs fit
static int enqueue_upload_plan(pbsgpu_engine *e, hipStream_t st, const UpPlan &up, uint64_t pieces_max) {
    const uint32_t nb = (up.n + 255) / 256;
    hipLaunchKernelGGL(pbsk::crc::k_upnew_count, dim3(nb), dim3(256), 0, st, up);
    hipLaunchKernelGGL(pbsk::crc::k_upnew_scan, dim3(1), dim3(256), 0, st, up);
    hipLaunchKernelGGL(pbsk::crc::k_upnew_fill, dim3(nb), dim3(256), 0, st, up);
    HIPCHK(hipGetLastError());
    if (pieces_max) {
        const uint64_t wg = std::min<uint64_t>((pieces_max + 255) / 256, (uint64_t)e->num_cus * 8);
        hipLaunchKernelGGL(pbsk::crc::k_upnew_ppart, dim3((unsigned)wg), dim3(256), 0, st, up);
        HIPCHK(hipGetLastError());
    }
    return PBSGPU_OK;
}

// with F_ZSTD the encoder's rounds over the live jobs, then the CRC pair on the plan's counts (its grids: the upper bounds
// the host knows)
static int enqueue_upload_blobs(pbsgpu_engine *e, hipStream_t st, const UploadSrc &src, uint8_t *dst, const UpBlock &ob,
                                const pbsk::zenc::Prep *zp, const UpDev &dv) {
    UpzPlan zl{};
    PartPlan &pl = zl.p;
    pl.base = src.base;
    pl.dst = dst;
    pl.parts = dv.up.parts;
    pl.blobs = dv.up.blobs;
    pl.ppart = dv.up.ppart;
    pl.praw = dv.praw;
    pl.crcs = reinterpret_cast<uint32_t *>(dv.out + ob.crcs);
    pl.counts = &dv.up.head->npieces;
    set_magic(pl);
    if (!zp) return launch_pair(e, st, k_pagecrc_pieces, k_pagecrc_fold, pl, src.pieces_max, dv.up.n);
    CHK(pbsk::zenc::launch(e, st, *zp, dv.room, src.base, dst, true));
    zl.res = dv.room.res;
    zl.lens = reinterpret_cast<uint32_t *>(dv.out + ob.lens);
    zl.kinds = dv.out + ob.kinds;
    zl.zmagic_lo = le32(kMagic[PBSGPU_BLOB_COMPRESSED]);
    zl.zmagic_hi = le32(kMagic[PBSGPU_BLOB_COMPRESSED] + 4);
    return launch_pair(e, st, k_upz_pieces, k_upz_fold, zl, src.pieces_max, dv.up.n);
}

// Order on the stream: mark -> (growth only: the number of new digests is read back and the table rebuilt) -> plan with
// the verdict -> insert with the plan's flags -> (F_ZSTD: the encoder's rounds over the live jobs) -> CRC pair on the
// plan's counts -> publish. The verdict comes before the insert and before the first byte of dst: when the blobs do not
// fit, the insert sees all-ones flags, no job is live and the pair sees zero counts, so the set and dst are as they were,
// while flags, stats and the size needed are already final.
int upload_new(pbsgpu_known *k, const UploadSrc &src, const pbsgpu_record *recs, uint64_t n, bool insert, uint32_t flags,
               uint8_t *dst, uint64_t dst_cap, uint8_t *known_out, uint64_t *blob_off, uint32_t *lens, uint8_t *kinds,
               uint32_t *crcs, uint64_t *used, pbsgpu_dedup_stats *stats, pbsgpu_encode_stats *enc) {
    pbsgpu_engine *e = known_engine(k);
    const bool zstd = (flags & PBSGPU_ENCODE_F_ZSTD) != 0;
    const auto size_of = [&](uint64_t i) { return src.chunks ? (uint32_t)src.chunks[i].length : recs[i].size; };
    std::vector<pbsk::zenc::Job> jobs;
    pbsk::zenc::Prep zp;
    if (zstd) {  // (before the lease: the one refusal left, 2^32 blocks, needs no device)
        jobs.resize((size_t)n);
        for (uint64_t i = 0; i < n; ++i) jobs[i] = pbsk::zenc::Job{0, 0, 0, size_of(i), size_of(i), 0, 0, pbsk::zenc::kNoJob};
        CHK(pbsk::zenc::prepare(e, jobs, src.chunks == nullptr, zp));
    }
    AuxLease lease(e);
    Slot *s = lease.s;
    const hipStream_t st = s->stream;
    const UpBlock ob((size_t)n, zstd);
    UpDev dv;
    CHK(stage_upload(s, src, recs, n, ob, zstd ? &zp : nullptr, jobs, dv));
    dv.up.dst_cap = dst_cap;
    CHK(known_enqueue_mark(k, dv.p, st));
    if (insert && known_may_grow(k, n)) {  // as known_common: the one case with a second synchronisation
        HIPCHK(hipMemcpyAsync(s->h_scalars.p, dv.p.stats, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        CHK(known_reserve(k, s->h_scalars.as<uint64_t>()[1], st));
    }
    CHK(enqueue_upload_plan(e, st, dv.up, src.pieces_max));
    if (insert) CHK(known_enqueue_insert(k, dv.p, dv.up.skip, st));
    CHK(enqueue_upload_blobs(e, st, src, dst, ob, zstd ? &zp : nullptr, dv));
    HIPCHK(pbsk::launch_publish(s->h_recs.p, dv.out, ob.total, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint8_t *h = s->h_recs.as<uint8_t>();
    UpHead head;
    std::memcpy(&head, h + ob.head, sizeof(head));
    const uint8_t *h_known = h + ob.known;
    if (known_out) std::memcpy(known_out, h_known, (size_t)n);
    if (stats) {
        stats->nrecords = head.stats[0];
        stats->nunique = head.stats[1];
        stats->total_bytes = head.stats[2];
        stats->unique_bytes = head.stats[3];
    }
    *used = head.total;
    if (head.over) return PBSGPU_E_CAPACITY;
    for (uint64_t i = 0, j = 0; i < n; ++i) {  // (crcs, lens and kinds are compacted: one per new record)
        if (h_known[i]) continue;
        std::memcpy(&blob_off[i], h + ob.boff + i * 8, 8);
        if (crcs) std::memcpy(&crcs[i], h + ob.crcs + j * 4, 4);
        uint32_t len = size_of(i) + PBSGPU_BLOB_HEADER_SIZE;
        uint8_t kind = PBSGPU_BLOB_UNCOMPRESSED;
        if (zstd) {
            std::memcpy(&len, h + ob.lens + j * 4, 4);
            kind = h[ob.kinds + j];
        }
        if (lens) lens[i] = len;
        if (kinds) kinds[i] = kind;
        if (enc) count_blob(*enc, kind, len, size_of(i));  // as pbsgpu_blob_encode2_device counts them
        ++j;
    }
    if (insert) known_inserted(k, head.stats[1]);
    return PBSGPU_OK;
}

}  // namespace pbse

extern "C" {

int pbsgpu_blob_magic(int kind, uint8_t out[8]) {
    if (!out || kind < 0 || kind > 3) return PBSGPU_E_INVALID;
    std::memcpy(out, kMagic[kind], 8);
    return PBSGPU_OK;
}

int pbsgpu_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t *out) {
    if (!out) return PBSGPU_E_INVALID;
    *out = mul(pow_from(kHost.x8, len_b), crc_a) ^ crc_b;
    return PBSGPU_OK;
}

int pbsgpu_crc32_many_device(pbsgpu_engine *e, const void *dptr, uint64_t nbytes, const pbsgpu_segment *segs,
                             uint32_t nseg, uint32_t *out) {
    return crc32_many(e, dptr, false, nbytes, segs, nseg, out);
}

int pbsgpu_crc32_many_host(pbsgpu_engine *e, const void *hptr, uint64_t nbytes, const pbsgpu_segment *segs, uint32_t nseg,
                           uint32_t *out) {
    return crc32_many(e, hptr, true, nbytes, segs, nseg, out);
}

int pbsgpu_blob_encoded_size(const pbsgpu_segment *segs, uint32_t nseg, uint64_t *nbytes) {
    if (!nbytes || (nseg && !segs)) return PBSGPU_E_INVALID;
    return encoded_size(segs, nseg, nbytes, nullptr);
}

int pbsgpu_blob_encode_device(pbsgpu_engine *e, const void *src, uint64_t src_bytes, const pbsgpu_segment *segs,
                              uint32_t nseg, void *dst, uint64_t dst_cap, uint64_t *out_len, uint64_t *offsets,
                              uint32_t *crcs) {
    if (!e || !out_len || (!src && src_bytes) || (nseg && !segs)) return PBSGPU_E_INVALID;
    if (!ranges_ok(segs, nseg, src_bytes)) return PBSGPU_E_INVALID;
    std::vector<uint64_t> offs((size_t)nseg + 1);
    uint64_t total = 0;
    CHK(encoded_size(segs, nseg, &total, offs.data()));
    *out_len = total;
    if (total > dst_cap) return PBSGPU_E_CAPACITY;
    if (offsets) std::memcpy(offsets, offs.data(), offs.size() * sizeof(uint64_t));
    if (nseg == 0) return PBSGPU_OK;
    if (!dst || !is_device_pointer(dst) || (src_bytes && !is_device_pointer(src))) return PBSGPU_E_INVALID;
    CHK(set_device(e));
    AuxLease lease(e);
    Slot *s = lease.s;
    const uint8_t *d = nullptr;
    CHK(stage_ranges(e, s, src, false, src_bytes, segs, nseg, &d));
    uint32_t *dcrcs = nullptr;
    CHK(enqueue_crc(e, s, d, segs, nseg, static_cast<uint8_t *>(dst), offs.data(), &dcrcs));
    if (crcs) return fetch_result(s, crcs, dcrcs, (size_t)nseg * 4);
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBSGPU_OK;
}

int pbsgpu_blob_encode2_device(pbsgpu_engine *e, const void *src, uint64_t src_bytes, const pbsgpu_segment *segs,
                               uint32_t nseg, uint32_t flags, void *dst, uint64_t dst_cap, uint64_t *offsets, uint32_t *lens,
                               uint8_t *kinds, uint32_t *crcs, pbsgpu_encode_stats *stats) {
    if (flags & ~PBSGPU_ENCODE_F_ZSTD) return PBSGPU_E_INVALID;
    if (!e || (!src && src_bytes) || (nseg && !segs)) return PBSGPU_E_INVALID;
    if (!ranges_ok(segs, nseg, src_bytes)) return PBSGPU_E_INVALID;
    for (uint32_t i = 0; i < nseg; ++i)
        if ((segs[i].length + PBSGPU_BLOB_HEADER_SIZE) >> 32) return PBSGPU_E_INVALID;  // lens is 32 bits wide
    std::vector<uint64_t> offs((size_t)nseg + 1);
    uint64_t total = 0;
    CHK(encoded_size(segs, nseg, &total, offs.data()));
    if (offsets) std::memcpy(offsets, offs.data(), offs.size() * sizeof(uint64_t));  // (also what a caller sizes dst with)
    if (total > dst_cap) return PBSGPU_E_CAPACITY;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    std::vector<uint32_t> vlens(nseg), vcrcs(nseg);
    std::vector<uint8_t> vkinds(nseg, (uint8_t)PBSGPU_BLOB_UNCOMPRESSED);
    if (!(flags & PBSGPU_ENCODE_F_ZSTD)) {
        uint64_t out_len = 0;
        CHK(pbsgpu_blob_encode_device(e, src, src_bytes, segs, nseg, dst, dst_cap, &out_len, nullptr, nseg ? vcrcs.data() : nullptr));
        for (uint32_t i = 0; i < nseg; ++i) vlens[i] = (uint32_t)(segs[i].length + PBSGPU_BLOB_HEADER_SIZE);
    } else if (nseg) {
        if (!dst || !is_device_pointer(dst) || (src_bytes && !is_device_pointer(src))) return PBSGPU_E_INVALID;
        if (overlaps(dst, total, src, src_bytes)) return PBSGPU_E_INVALID;  // the frames are read back
        CHK(set_device(e));
        CHK(blob_encode_zstd(e, static_cast<const uint8_t *>(src), segs, nseg, static_cast<uint8_t *>(dst), offs.data(), src_bytes,
                             vlens.data(), vkinds.data(), vcrcs.data()));
    }
    if (stats)
        for (uint32_t i = 0; i < nseg; ++i) count_blob(*stats, vkinds[i], vlens[i], segs[i].length);
    if (lens && nseg) std::memcpy(lens, vlens.data(), (size_t)nseg * 4);
    if (kinds && nseg) std::memcpy(kinds, vkinds.data(), nseg);
    if (crcs && nseg) std::memcpy(crcs, vcrcs.data(), (size_t)nseg * 4);
    return PBSGPU_OK;
}

int pbsgpu_blob_encoded_size3(const pbsgpu_segment *segs, uint32_t nseg, uint32_t flags, uint64_t *nbytes) {
    if (!nbytes || (nseg && !segs) || (flags & ~(PBSGPU_ENCODE_F_ZSTD | PBSGPU_ENCODE_F_AES))) return PBSGPU_E_INVALID;
    const uint32_t hdr = (flags & PBSGPU_ENCODE_F_AES) ? PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE : PBSGPU_BLOB_HEADER_SIZE;
    return slot_offsets(segs, nseg, hdr, nullptr, nbytes) ? PBSGPU_OK : PBSGPU_E_INVALID;
}

int pbsgpu_blob_encode3_device(pbsgpu_engine *e, const void *src, uint64_t src_bytes, const pbsgpu_segment *segs,
                               uint32_t nseg, uint32_t flags, pbsgpu_aes_key *key, const uint8_t *ivs, void *dst,
                               uint64_t dst_cap, uint64_t *offsets, uint32_t *lens, uint8_t *kinds, uint32_t *crcs,
                               pbsgpu_encode_stats3 *stats) {
    if (flags & ~(PBSGPU_ENCODE_F_ZSTD | PBSGPU_ENCODE_F_AES)) return PBSGPU_E_INVALID;
    if (!(flags & PBSGPU_ENCODE_F_AES)) {  // the older call, output for output; key and ivs are not looked at
        pbsgpu_encode_stats st2{};
        CHK(pbsgpu_blob_encode2_device(e, src, src_bytes, segs, nseg, flags, dst, dst_cap, offsets, lens, kinds, crcs,
                                       stats ? &st2 : nullptr));
        if (stats) {
            std::memset(stats, 0, sizeof(*stats));
            for (int k = 0; k < 2; ++k) {
                stats->blobs[k] = st2.blobs[k];
                stats->blob_bytes[k] = st2.blob_bytes[k];
                stats->chunk_bytes[k] = st2.chunk_bytes[k];
            }
            stats->frame_bytes = st2.frame_bytes;
            stats->crc_bytes = st2.crc_bytes;
        }
        return PBSGPU_OK;
    }
    if (!e || (!src && src_bytes) || (nseg && !segs)) return PBSGPU_E_INVALID;
    if (!ranges_ok(segs, nseg, src_bytes)) return PBSGPU_E_INVALID;
    for (uint32_t i = 0; i < nseg; ++i)
        if ((segs[i].length + PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE) >> 32) return PBSGPU_E_INVALID;  // lens is 32 bits wide
    if (!key || pbsk::aes::key_engine(key) != e || (nseg && !ivs)) return PBSGPU_E_INVALID;
    if (!ivs_distinct(ivs, nseg)) return PBSGPU_E_INVALID;
    std::vector<uint64_t> offs((size_t)nseg + 1);
    uint64_t total = 0;
    if (!slot_offsets(segs, nseg, PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE, offs.data(), &total)) return PBSGPU_E_INVALID;
    if (offsets) std::memcpy(offsets, offs.data(), offs.size() * sizeof(uint64_t));  // (also what a caller sizes dst with)
    if (total > dst_cap) return PBSGPU_E_CAPACITY;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (nseg == 0) return PBSGPU_OK;
    if (!dst || overlaps(dst, total, src, src_bytes)) return PBSGPU_E_INVALID;  // a frame is encrypted where it lies
    CHK(set_device(e));
    if (!is_device_pointer(dst) || (src_bytes && !is_device_pointer(src))) return PBSGPU_E_INVALID;
    std::vector<uint32_t> vlens(nseg), vcrcs(nseg);
    std::vector<uint8_t> vkinds(nseg);
    CHK(blob_encode_aes(e, key, ivs, (flags & PBSGPU_ENCODE_F_ZSTD) != 0, static_cast<const uint8_t *>(src), segs, nseg,
                        static_cast<uint8_t *>(dst), offs.data(), src_bytes, vlens.data(), vkinds.data(), vcrcs.data()));
    if (stats)
        for (uint32_t i = 0; i < nseg; ++i) count_blob3(*stats, vkinds[i], vlens[i], segs[i].length);
    if (lens) std::memcpy(lens, vlens.data(), (size_t)nseg * 4);
    if (kinds) std::memcpy(kinds, vkinds.data(), nseg);
    if (crcs) std::memcpy(crcs, vcrcs.data(), (size_t)nseg * 4);
    return PBSGPU_OK;
}

int pbsgpu_blob_verify_device(pbsgpu_engine *e, const void *dptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                              uint32_t nblob, const uint8_t *digests, const uint32_t *sizes, uint8_t *status,
                              pbsgpu_blob_stats *stats) {
    return blob_verify(e, dptr, false, nbytes, blobs, nblob, digests, sizes, status, stats);
}

int pbsgpu_blob_verify_host(pbsgpu_engine *e, const void *hptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                            uint32_t nblob, const uint8_t *digests, const uint32_t *sizes, uint8_t *status,
                            pbsgpu_blob_stats *stats) {
    return blob_verify(e, hptr, true, nbytes, blobs, nblob, digests, sizes, status, stats);
}

int pbsgpu_blob_decode_device(pbsgpu_engine *e, const void *blobs_dptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                              uint32_t nblob, const pbsgpu_record *idx, uint64_t nidx, const uint32_t *blob_of,
                              uint64_t range_start, uint64_t range_end, int check_digest, void *dst, uint64_t dst_cap,
                              uint8_t *status, pbsgpu_decode_stats *stats) {
    pbsgpu_decode_stats3 st2{};
    const int r = blob_decode(e, blobs_dptr, nbytes, blobs, nblob, idx, nidx, blob_of, range_start, range_end,
                              check_digest ? PBSGPU_DECODE_F_DIGEST : 0u, nullptr, dst, dst_cap, status, &st2);
    if (stats && e && nidx < (1ull << 32)) {  // (past those two checks the statistics are cleared first, as they always were)
        for (int k = 0; k < PBSGPU_BLOB_NSTATUS; ++k) stats->count[k] = st2.count[k];
        stats->blob_bytes = st2.blob_bytes;
        stats->crc_bytes = st2.crc_bytes;
        stats->sha_bytes = st2.sha_bytes;
        stats->out_bytes = st2.out_bytes;
    }
    return r;
}

int pbsgpu_blob_decode2_device(pbsgpu_engine *e, const void *blobs_dptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                               uint32_t nblob, const pbsgpu_record *idx, uint64_t nidx, const uint32_t *blob_of,
                               uint64_t range_start, uint64_t range_end, uint32_t flags, void *dst, uint64_t dst_cap,
                               uint8_t *status, pbsgpu_decode_stats2 *stats) {
    if (flags & ~(PBSGPU_DECODE_F_DIGEST | PBSGPU_DECODE_F_ZSTD)) return PBSGPU_E_INVALID;
    pbsgpu_decode_stats3 st3{};
    const int r = blob_decode(e, blobs_dptr, nbytes, blobs, nblob, idx, nidx, blob_of, range_start, range_end, flags, nullptr, dst,
                              dst_cap, status, stats ? &st3 : nullptr);
    static_assert(sizeof(pbsgpu_decode_stats3) == sizeof(pbsgpu_decode_stats2) + 8, "stats3 is stats2 and one field more");
    if (stats && e && nidx < (1ull << 32)) std::memcpy(stats, &st3, sizeof(*stats));  // (cleared past those two checks, as ever)
    return r;
}

int pbsgpu_blob_decode3_device(pbsgpu_engine *e, const void *blobs_dptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                               uint32_t nblob, const pbsgpu_record *idx, uint64_t nidx, const uint32_t *blob_of,
                               uint64_t range_start, uint64_t range_end, uint32_t flags, pbsgpu_aes_key *key, void *dst,
                               uint64_t dst_cap, uint8_t *status, pbsgpu_decode_stats3 *stats) {
    if (flags & ~(PBSGPU_DECODE_F_DIGEST | PBSGPU_DECODE_F_ZSTD | PBSGPU_DECODE_F_AES)) return PBSGPU_E_INVALID;
    return blob_decode(e, blobs_dptr, nbytes, blobs, nblob, idx, nidx, blob_of, range_start, range_end, flags, key, dst, dst_cap,
                       status, stats);
}

int pbsgpu_blob_decode4_device(pbsgpu_engine *e, const void *blobs_dptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                               uint32_t nblob, const pbsgpu_record *idx, uint64_t nidx, const uint32_t *blob_of,
                               uint64_t range_start, uint64_t range_end, uint32_t flags, pbsgpu_aes_key *key, pbsgpu_id_key *idkey,
                               void *dst, uint64_t dst_cap, uint8_t *status, pbsgpu_decode_stats3 *stats) {
    if (flags & ~(PBSGPU_DECODE_F_DIGEST | PBSGPU_DECODE_F_ZSTD | PBSGPU_DECODE_F_AES)) return PBSGPU_E_INVALID;
    return blob_decode(e, blobs_dptr, nbytes, blobs, nblob, idx, nidx, blob_of, range_start, range_end, flags, key, dst, dst_cap,
                       status, stats, idkey);
}

int pbsgpu_known_upload_new2_device(pbsgpu_known *k, const void *src, uint64_t src_bytes, const pbsgpu_record *recs,
                                    const pbsgpu_segment *chunks, uint64_t n, int insert, uint32_t flags, void *dst,
                                    uint64_t dst_cap, uint8_t *known_out, uint64_t *blob_off, uint32_t *lens, uint8_t *kinds,
                                    uint32_t *crcs, uint64_t *used, pbsgpu_dedup_stats *stats, pbsgpu_encode_stats *enc_stats) {
    if (flags & ~PBSGPU_ENCODE_F_ZSTD) return PBSGPU_E_INVALID;
    if (!k || !used || !stats || (!src && src_bytes) || (n && (!recs || !chunks || !blob_off)) || n >= (1ull << 32))
        return PBSGPU_E_INVALID;
    if (!dst && dst_cap) return PBSGPU_E_INVALID;
    UploadSrc us;
    for (uint64_t i = 0; i < n; ++i) {  // every chunk, not only the new ones: which ones are new is not known here
        const pbsgpu_segment &c = chunks[i];
        if (c.length > src_bytes || c.offset > src_bytes - c.length || c.length >= (1ull << 31)) return PBSGPU_E_INVALID;
        us.pieces_max += pbsp::pieces_of(c.length);
    }
    if (us.pieces_max >= (1ull << 32)) return PBSGPU_E_INVALID;
    if ((flags & PBSGPU_ENCODE_F_ZSTD) && overlaps(dst, dst_cap, src, src_bytes))  // the frames are read again for their CRC
        return PBSGPU_E_INVALID;
    *used = 0;
    std::memset(stats, 0, sizeof(*stats));
    if (enc_stats) std::memset(enc_stats, 0, sizeof(*enc_stats));
    if (n == 0) return PBSGPU_OK;
    CHK(set_device(known_engine(k)));
    if ((dst && !is_device_pointer(dst)) || (src_bytes && !is_device_pointer(src))) return PBSGPU_E_INVALID;
    us.base = static_cast<const uint8_t *>(src);
    us.chunks = chunks;
    return upload_new(k, us, recs, n, insert != 0, flags, static_cast<uint8_t *>(dst), dst_cap, known_out, blob_off, lens,
                      kinds, crcs, used, stats, enc_stats);
}

int pbsgpu_known_upload_new_device(pbsgpu_known *k, const void *src, uint64_t src_bytes, const pbsgpu_record *recs,
                                   const pbsgpu_segment *chunks, uint64_t n, int insert, void *dst, uint64_t dst_cap,
                                   uint8_t *known_out, uint64_t *blob_off, uint32_t *crcs, uint64_t *used,
                                   pbsgpu_dedup_stats *stats) {
    return pbsgpu_known_upload_new2_device(k, src, src_bytes, recs, chunks, n, insert, 0, dst, dst_cap, known_out, blob_off,
                                           nullptr, nullptr, crcs, used, stats, nullptr);
}

}  // extern "C"
