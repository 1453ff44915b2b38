// Zstandard frame decoding (RFC 8878) for the restore path: ONE implementation, compiled twice. Under hipcc every
// function is __host__ __device__ and zstd.hip runs it with one wave per frame; without hipcc it is plain inline C++, and
// that build is what tests/native/test_zstd_core.cpp fuzzes under AddressSanitizer and pbsgpu_zstd_frame_info
// (hostonly.cpp) uses. No HIP and no libc beyond the fixed-width integers.
//
// Everything that decides about bytes is here: frame and block headers, the literals section, Huffman weights, FSE
// tables, the sequences section, the repeat offsets, and every bound. A caller adds only the cooperation between lanes,
// as a policy P:
//   P::lane()   this lane's number, 0 <= lane < P::lanes()
//   P::lanes()  how many lanes run decode_frame together (1 on the host, 64 in the kernel)
//   P::sync()   all lanes have arrived and every store made before is visible to every lane after
//   P::uni(v)   v, which every lane holds alike, as a value the compiler knows to be the same in all lanes
// All lanes call decode_frame with the same arguments and walk the same control flow. What is serial by nature (table
// builds, the FSE chain of the sequences) runs on lane 0 and is handed over through State; copies and fills are strided
// over the lanes; the four Huffman streams of a literals section run on four lanes.
//
// Decisions (include/pbsgpu.h):
//   * The content checksum (XXH64, another serial chain per chunk) is parsed and accounted for, NOT verified by
//     decode_frame: the blob's CRC-32 covers the compressed bytes and the index digest covers the content. The
//     stand-alone call that is asked to verifies it (zstd_stream.h, pbsgpu_zstd_decode2_device).
//   * A nonzero dictionary id, a skippable frame, a second frame or trailing bytes are UNSUPPORTED: a blob is one frame.
//     (Whole streams: zstd_stream.h, for the same stand-alone call.)
//   * An offset is valid iff it does not reach before the frame's first output byte: the decoder writes straight into
//     the destination, so the output so far is the window. A declared window size is read, not enforced, not allocated.
//   * The decoder knows the room it may write and never stores outside it: a declared content size above the room is
//     refused before anything is written, and every copy is checked against the room before it is made.
//   * Every table index, bit position and length is checked before use: reading past either end of a backward bit
//     stream, an FSE distribution that does not sum, an incomplete Huffman weight set are BAD_FRAME.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define PBSZ_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PBSZ_HD inline
#endif

// in front of a short serial loop: left rolled and scalar. Unrolled, the kernel keeps a constant table in registers, or the
// lane masks of eight iterations in SGPR pairs, and spills
#if defined(__clang__)
#define PBSZ_ROLLED _Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
#elif defined(__GNUC__)
#define PBSZ_ROLLED _Pragma("GCC unroll 1")
#else
#define PBSZ_ROLLED
#endif

#ifdef PBSGPU_ZSTD_COVERAGE  // CPU test build only: one bit per format branch (names: tests/native/test_zstd_core.cpp)
namespace pbsz {
inline uint64_t g_cov = 0;
}
#define PBSZ_COV(bit) (::pbsz::g_cov |= 1ull << (bit))
#define PBSZ_COV_IF(cond, bit) ((cond) ? (void)PBSZ_COV(bit) : (void)0)
#else
#define PBSZ_COV(bit) ((void)0)
#define PBSZ_COV_IF(cond, bit) ((void)0)  // the condition is not compiled either: the kernel is what it was
#endif

namespace pbsz {

enum : int { OK = 0, BAD_FRAME = 1, BAD_SIZE = 2, UNSUPPORTED = 3 };

enum : int {  // coverage bits
    C_SINGLE_SEGMENT, C_WINDOW_DESC, C_FCS_1, C_FCS_2, C_FCS_4, C_FCS_8, C_FCS_ABSENT, C_CHECKSUM, C_NO_CHECKSUM,
    C_BLOCK_RAW, C_BLOCK_RLE, C_BLOCK_COMPRESSED, C_MANY_BLOCKS, C_EMPTY_LAST_BLOCK,
    C_LIT_RAW_1, C_LIT_RAW_2, C_LIT_RAW_3, C_LIT_RLE_1, C_LIT_RLE_2, C_LIT_RLE_3,
    C_HUF_1STREAM, C_HUF_4STREAM_3, C_HUF_4STREAM_4, C_HUF_4STREAM_5, C_HUF_TREELESS, C_WEIGHTS_DIRECT, C_WEIGHTS_FSE,
    C_NSEQ_0, C_NSEQ_1, C_NSEQ_2, C_NSEQ_3,
    C_LL_PREDEF, C_LL_RLE, C_LL_FSE, C_LL_REPEAT, C_OF_PREDEF, C_OF_RLE, C_OF_FSE, C_OF_REPEAT,
    C_ML_PREDEF, C_ML_RLE, C_ML_FSE, C_ML_REPEAT,
    C_REP_1, C_REP_2, C_REP_3, C_REP_SHIFTED, C_REP_1_MINUS_1, C_MATCH_OVERLAP, C_MATCH_OFFSET_1, C_MATCH_ACROSS_BLOCKS,
    // where the lanes of the kernel cooperate (the CPU build walks the same branches with one lane): a match that waits
    // for the stores before it and one that does not, a source inside the match just before and inside the sequence's
    // own literal run, a literal run copied by one lane and by all, a batch whose first match reads the last match of
    // the batch before
    C_MATCH_WAIT, C_MATCH_NO_WAIT, C_MATCH_SRC_IN_PREV_MATCH, C_MATCH_SRC_OWN_LITERALS, C_LIT_SHORT, C_LIT_LONG,
    C_BATCH_FOLLOWS_BATCH,
    // what only crafted Huffman literals and table descriptions reach (tests/zstd_huf_inputs.py): a stream that ends with
    // spare bits, codes of kHufLogMax bits, a fourth stream shorter than the other three, the weights' FSE stream ending
    // on its first and on its second state, a zero run in a table description that goes on after a count of 3
    C_HUF_SPARE_BITS, C_HUF_LOG_MAX, C_HUF_SHORT_4TH, C_WEIGHTS_END_FIRST, C_WEIGHTS_END_SECOND, C_NORM_ZERO_RUN_CHAINED,
    C_NBITS
};

constexpr uint32_t kLitMax = 128u << 10;  // a block's literals: the size of the literal buffer the caller passes
constexpr uint32_t kBlockMax = 128u << 10;
constexpr int kBatch = 64;                // sequences resolved by lane 0 before the lanes execute them
constexpr uint64_t kNoSize = ~0ull;
constexpr int kHufLogMax = 12;            // the reference decoder takes 12 although an encoder stops at 11

struct FrameHeader {
    uint64_t content_size;  // kNoSize: not declared
    uint64_t window_size;
    uint32_t header_bytes;
    uint32_t has_checksum;
};

struct FseEntry {
    uint16_t next;
    uint8_t sym;
    uint8_t nbits;
};

struct Seq {
    uint32_t out;  // where its literals go
    uint32_t lit;  // where they come from
    uint32_t ll, ml, off;
};

// Per frame in flight: 8 KiB Huffman table, 5 KiB FSE tables, the batch, the build scratch. LDS in the kernel.
struct State {
    uint16_t huf[1 << kHufLogMax];  // symbol | nbits << 8
    FseEntry ll[512], of[256], ml[512];
    FseEntry wt[64];                // the FSE table of compressed Huffman weights
    Seq seq[kBatch];
    int16_t norm[256];
    uint16_t next[256];
    uint8_t weights[256];
    uint32_t rank[kHufLogMax + 2];
    uint32_t rep[3];
    uint32_t huf_log, ll_log, of_log, ml_log;
    uint32_t huf_valid, ll_valid, of_valid, ml_valid;
    uint32_t tmp, litpos;
    int32_t err;
    uint32_t out;
};

// sequence codes -> baseline and extra bits
constexpr uint32_t kLLBase[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,   9,   10,  11,   12,   13,   14,    15,    16,    18,
                                  20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
constexpr uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
constexpr uint32_t kMLBase[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16,  17,  18,  19,   20,
                                  21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,  35,  37,  39,   41,
                                  43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
constexpr uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
// predefined distributions
constexpr int8_t kLLDefault[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                   2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
constexpr int8_t kMLDefault[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
constexpr int8_t kOFDefault[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};

PBSZ_HD uint32_t highbit(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }  // x != 0

PBSZ_HD uint64_t load_le(const uint8_t *p, uint32_t nb) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < nb; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

struct HostLanes {  // the policy of a plain CPU caller
    static PBSZ_HD int lane() { return 0; }
    static PBSZ_HD int lanes() { return 1; }
    static PBSZ_HD void sync() {}
    static PBSZ_HD uint32_t uni(uint32_t v) { return v; }
};

// a value every lane holds alike, said so to the compiler: what branches on it is a scalar branch, not a lane mask
template <class P>
PBSZ_HD uint64_t uload(const uint8_t *p, uint32_t nb) {
    const uint64_t v = load_le(p, nb);
    return (uint64_t)P::uni((uint32_t)v) | (uint64_t)(nb > 4 ? P::uni((uint32_t)(v >> 32)) : 0u) << 32;
}

// The frame header alone: what pbsgpu_zstd_frame_info reports.
template <class P = HostLanes>
PBSZ_HD int parse_frame_header(const uint8_t *src, uint64_t n, FrameHeader &h) {
    h.content_size = kNoSize;
    h.window_size = 0;
    h.header_bytes = 0;
    h.has_checksum = 0;
    if (n < 4) return BAD_FRAME;
    const uint32_t magic = (uint32_t)uload<P>(src, 4);
    if ((magic & 0xfffffff0u) == 0x184d2a50u) return UNSUPPORTED;  // a skippable frame
    if (magic != 0xfd2fb528u) return BAD_FRAME;
    if (n < 5) return BAD_FRAME;
    const uint32_t fhd = P::uni(src[4]);
    if (fhd & 8u) return BAD_FRAME;  // reserved bit
    const uint32_t single = (fhd >> 5) & 1u, fcs_flag = fhd >> 6, did_flag = fhd & 3u;
    const uint32_t wd = single ? 0u : 1u;
    const uint32_t did = did_flag == 3 ? 4u : did_flag;
    const uint32_t fcs = fcs_flag == 0 ? single : (1u << fcs_flag);
    const uint32_t hb = 5 + wd + did + fcs;
    if (n < hb) return BAD_FRAME;
    uint32_t p = 5;
    if (wd) {
        const uint32_t b = P::uni(src[p++]);
        const uint64_t base = 1ull << (10 + (b >> 3));
        h.window_size = base + (base >> 3) * (b & 7u);
    }
    if (did && uload<P>(src + p, did) != 0) return UNSUPPORTED;  // a dictionary
    p += did;
    if (fcs) {
        h.content_size = uload<P>(src + p, fcs);
        if (fcs == 2) h.content_size += 256;
    }
    if (single) h.window_size = h.content_size;
    h.header_bytes = hb;
    h.has_checksum = (fhd >> 2) & 1u;
    PBSZ_COV(single ? C_SINGLE_SEGMENT : C_WINDOW_DESC);
    PBSZ_COV(fcs == 0 ? C_FCS_ABSENT : fcs == 1 ? C_FCS_1 : fcs == 2 ? C_FCS_2 : fcs == 4 ? C_FCS_4 : C_FCS_8);
    PBSZ_COV(h.has_checksum ? C_CHECKSUM : C_NO_CHECKSUM);
    return OK;
}

// A backward bit stream: bytes p[0, n), read from the top bit below the end mark of the last byte down to bit 0 of p[0].
// pos = bits left. Bits below bit 0 read as zero and set `over`; no byte outside [0, n) is ever loaded. The 64-bit window
// holds the bytes [wbit / 8, wbit / 8 + 8) and is reloaded when a read leaves it.
struct BitReader {
    const uint8_t *p;
    int32_t n, pos, wbit;
    uint64_t win;
    bool over;

    PBSZ_HD bool init(const uint8_t *src, uint32_t len) {  // len <= kBlockMax
        p = src;
        n = (int32_t)len;
        over = false;
        win = 0;
        pos = 0;
        wbit = 1;
        if (len == 0) return false;
        const uint32_t last = src[len - 1];
        if (last == 0) return false;
        pos = (int32_t)((len - 1) * 8 + highbit(last));
        wbit = pos + 1;  // forces the first load
        return true;
    }
    PBSZ_HD uint32_t peek(uint32_t k) {  // the next k <= 32 bits, zero-filled below bit 0
        if (k == 0) return 0;
        const int32_t s = pos - (int32_t)k;
        if (s < wbit || pos > wbit + 64) {
            const int32_t wbyte = ((pos + 7) >> 3) - 8;  // pos >= 0 here
            uint64_t w = 0;
            for (int i = 0; i < 8; ++i) {
                const int32_t b = wbyte + i;
                if (b >= 0 && b < n) w |= (uint64_t)p[b] << (8 * i);
            }
            win = w;
            wbit = wbyte * 8;
        }
        return (uint32_t)((win >> (s - wbit)) & ((1ull << k) - 1));
    }
    PBSZ_HD void skip(uint32_t k) {
        pos -= (int32_t)k;
        if (pos < 0) {
            over = true;
            pos = 0;
        }
    }
    PBSZ_HD uint32_t read(uint32_t k) {
        if (over) return 0;
        const uint32_t v = peek(k);
        skip(k);
        return v;
    }
};

// An FSE table description (forward bit stream) into st.norm[0 .. *nsym). BAD_FRAME unless the probabilities sum to
// 1 << log exactly, log <= max_log and no symbol above max_sym is named. *used = bytes consumed.
PBSZ_HD int fse_read_norm(State &st, const uint8_t *p, uint32_t len, uint32_t max_log, uint32_t max_sym, uint32_t *log,
                          uint32_t *nsym, uint32_t *used) {
    uint32_t bit = 0;
    const uint32_t nbit = len * 8;  // len <= kBlockMax
    auto rd = [&](uint32_t k, uint32_t *v) -> bool {  // 0 < k <= 16
        if (nbit - bit < k) return false;
        const uint32_t b = bit >> 3, end = len - 1;  // the bits asked for end inside p[0, len): a byte index clamped to
        const uint32_t b1 = b + 1 < end ? b + 1 : end, b2 = b + 2 < end ? b + 2 : end;  // `end` only feeds bits masked off
        const uint32_t w = (uint32_t)p[b] | (uint32_t)p[b1] << 8 | (uint32_t)p[b2] << 16;
        *v = (w >> (bit & 7)) & ((1u << k) - 1);
        bit += k;
        return true;
    };
    uint32_t v;
    if (!rd(4, &v)) return BAD_FRAME;
    const uint32_t al = v + 5;
    if (al > max_log) return BAD_FRAME;
    int32_t remaining = 1 << al;
    uint32_t sym = 0;
    while (remaining > 0 && sym <= max_sym) {
        const uint32_t bits = highbit((uint32_t)remaining + 1) + 1;
        if (!rd(bits, &v)) return BAD_FRAME;
        const uint32_t lower = (1u << (bits - 1)) - 1;
        const uint32_t threshold = (1u << bits) - 1 - ((uint32_t)remaining + 1);
        if ((v & lower) < threshold) {
            bit -= 1;
            v &= lower;
        } else if (v > lower) {
            v -= threshold;
        }
        const int32_t proba = (int32_t)v - 1;
        remaining -= proba < 0 ? 1 : proba;
        st.norm[sym++] = (int16_t)proba;
        if (proba == 0) {
            for (;;) {
                uint32_t rep;
                if (!rd(2, &rep)) return BAD_FRAME;
                for (uint32_t i = 0; i < rep; ++i) {
                    if (sym > max_sym) return BAD_FRAME;
                    st.norm[sym++] = 0;
                }
                if (rep != 3) break;
                PBSZ_COV(C_NORM_ZERO_RUN_CHAINED);
            }
        }
    }
    if (remaining != 0) return BAD_FRAME;  // too many symbols, or probabilities that overshoot
    *log = al;
    *nsym = sym;
    *used = (bit + 7) >> 3;
    return OK;
}

// The decoding table of st.norm[0, nsym) with accuracy log `log`; tab has 1 << log entries.
PBSZ_HD int fse_build(State &st, FseEntry *tab, uint32_t log, uint32_t nsym) {
    const uint32_t size = 1u << log, mask = size - 1;
    uint32_t high = size;
    for (uint32_t s = 0; s < nsym; ++s) {
        if (st.norm[s] == -1) {
            if (high == 0) return BAD_FRAME;
            tab[--high].sym = (uint8_t)s;
            st.next[s] = 1;
        } else {
            st.next[s] = (uint16_t)st.norm[s];
        }
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
        for (int32_t i = 0; i < st.norm[s]; ++i) {
            if (pos >= high) return BAD_FRAME;  // (cannot happen when the probabilities sum; keeps the index bounded)
            tab[pos].sym = (uint8_t)s;
            do pos = (pos + step) & mask;
            while (pos >= high && pos != 0);
        }
    }
    if (pos != 0) return BAD_FRAME;
    for (uint32_t u = 0; u < size; ++u) {
        const uint32_t s = tab[u].sym;
        const uint32_t nx = st.next[s]++;
        if (nx == 0) return BAD_FRAME;
        const uint32_t nb = log - highbit(nx);
        tab[u].nbits = (uint8_t)nb;
        tab[u].next = (uint16_t)((nx << nb) - size);
    }
    return OK;
}

// The Huffman tree description at p[0, len): the weights (direct or FSE-compressed), the implied last weight, the table.
PBSZ_HD int huf_read_table(State &st, const uint8_t *p, uint32_t len, uint32_t *used) {
    st.huf_valid = 0;
    if (len < 1) return BAD_FRAME;
    const uint32_t h = p[0];
    uint32_t nw = 0;
    if (h >= 128) {
        PBSZ_COV(C_WEIGHTS_DIRECT);
        nw = h - 127;
        const uint32_t bytes = (nw + 1) / 2;
        if (len - 1 < bytes) return BAD_FRAME;
        PBSZ_ROLLED
        for (uint32_t i = 0; i < nw; ++i) st.weights[i] = (i & 1) ? (p[1 + i / 2] & 15u) : (p[1 + i / 2] >> 4);
        *used = 1 + bytes;
    } else {
        PBSZ_COV(C_WEIGHTS_FSE);
        if (h == 0 || len - 1 < h) return BAD_FRAME;
        uint32_t log, nsym, cons;
        int r = fse_read_norm(st, p + 1, h, 6, 255, &log, &nsym, &cons);
        if (r) return r;
        r = fse_build(st, st.wt, log, nsym);
        if (r) return r;
        BitReader br;
        if (cons >= h || !br.init(p + 1 + cons, h - cons)) return BAD_FRAME;
        uint32_t s1 = br.read(log), s2 = br.read(log);
        if (br.over) return BAD_FRAME;
        for (;;) {  // two interleaved states until the stream runs out: the other state's symbol is the last
            if (nw + 2 > 255) return BAD_FRAME;  // 255 weights at most: the implied one makes 256 symbols
            st.weights[nw++] = st.wt[s1].sym;
            s1 = st.wt[s1].next + br.read(st.wt[s1].nbits);
            if (br.over) {
                st.weights[nw++] = st.wt[s2].sym;
                PBSZ_COV((nw & 1) ? C_WEIGHTS_END_FIRST : C_WEIGHTS_END_SECOND);  // (the roles swapped nw - 1 times)
                break;
            }
            const uint32_t t = s1;  // the roles swap
            s1 = s2;
            s2 = t;
        }
        *used = 1 + h;
    }
    uint32_t total = 0;
    PBSZ_ROLLED
    for (uint32_t w = 0; w < kHufLogMax + 2; ++w) st.rank[w] = 0;
    for (uint32_t i = 0; i < nw; ++i) {
        const uint32_t w = st.weights[i];
        if (w > kHufLogMax) return BAD_FRAME;
        if (w) total += 1u << (w - 1);
        st.rank[w]++;
    }
    if (total == 0) return BAD_FRAME;
    const uint32_t log = highbit(total) + 1;
    if (log > kHufLogMax) return BAD_FRAME;
    const uint32_t rest = (1u << log) - total;  // >= 1
    if (rest & (rest - 1)) return BAD_FRAME;    // the weights do not complete to a power of two
    const uint32_t lastw = highbit(rest) + 1;
    st.weights[nw++] = (uint8_t)lastw;  // nw <= 256
    st.rank[lastw]++;
    uint32_t start = 0;  // first table index of each weight: weight 1 (the longest codes) first
    for (uint32_t w = 1; w <= log; ++w) {
        const uint32_t cnt = st.rank[w];
        st.rank[w] = start;
        start += cnt << (w - 1);
    }
    if (start != (1u << log)) return BAD_FRAME;
    for (uint32_t s = 0; s < nw; ++s) {
        const uint32_t w = st.weights[s];
        if (!w) continue;
        const uint32_t cnt = 1u << (w - 1), at = st.rank[w];
        const uint16_t e = (uint16_t)(s | (log + 1 - w) << 8);
        for (uint32_t i = 0; i < cnt; ++i) st.huf[at + i] = e;
        st.rank[w] = at + cnt;
    }
    PBSZ_COV_IF(log == kHufLogMax, C_HUF_LOG_MAX);
    st.huf_log = log;
    st.huf_valid = 1;
    return OK;
}

// One Huffman stream p[0, len) into out[0, nout): no bit beyond the stream is read. Fewer spare bits than one table lookup
// may stay unused: the reference decoder's double-symbol path takes them with its last lookup, so such frames exist.
PBSZ_HD int huf_stream(const State &st, const uint8_t *p, uint32_t len, uint8_t *out, uint32_t nout) {
    BitReader br;
    if (!br.init(p, len)) return BAD_FRAME;
    const uint32_t log = st.huf_log;
    for (uint32_t i = 0; i < nout; ++i) {
        const uint32_t e = st.huf[br.peek(log)];
        br.skip(e >> 8);
        if (br.over) return BAD_FRAME;
        out[i] = (uint8_t)e;
    }
    PBSZ_COV_IF(br.pos > 0 && br.pos < (int32_t)log, C_HUF_SPARE_BITS);
    return br.pos < (int32_t)log ? OK : BAD_FRAME;
}

template <class P>
PBSZ_HD void copy_bytes(uint8_t *dst, const uint8_t *src, uint32_t n) {
    for (uint32_t i = (uint32_t)P::lane(); i < n; i += (uint32_t)P::lanes()) dst[i] = src[i];
}

template <class P>
PBSZ_HD void fill_bytes(uint8_t *dst, uint8_t v, uint32_t n) {
    for (uint32_t i = (uint32_t)P::lane(); i < n; i += (uint32_t)P::lanes()) dst[i] = v;
}

// One of the three sequence tables (lane 0). which: 0 literal lengths, 1 offsets, 2 match lengths.
PBSZ_HD int seq_table(State &st, uint32_t which, uint32_t mode, const uint8_t *b, uint32_t bs, uint32_t *p) {
    FseEntry *tab = which == 0 ? st.ll : which == 1 ? st.of : st.ml;
    uint32_t *log = which == 0 ? &st.ll_log : which == 1 ? &st.of_log : &st.ml_log;
    uint32_t *valid = which == 0 ? &st.ll_valid : which == 1 ? &st.of_valid : &st.ml_valid;
    const uint32_t max_sym = which == 0 ? 35u : which == 1 ? 31u : 52u;
    const uint32_t max_log = which == 1 ? 8u : 9u;
    PBSZ_COV((which == 0 ? C_LL_PREDEF : which == 1 ? C_OF_PREDEF : C_ML_PREDEF) + (int)mode);
    if (mode == 3) return *valid ? OK : BAD_FRAME;  // repeat: the previous block's table
    *valid = 0;
    if (mode == 0) {
        const uint32_t n = which == 0 ? 36u : which == 1 ? 29u : 53u;
        PBSZ_ROLLED
        for (uint32_t s = 0; s < n; ++s) st.norm[s] = which == 0 ? kLLDefault[s] : which == 1 ? kOFDefault[s] : kMLDefault[s];
        *log = which == 1 ? 5u : 6u;
        const int r = fse_build(st, tab, *log, n);
        if (r) return r;
    } else if (mode == 1) {
        if (*p >= bs) return BAD_FRAME;
        const uint32_t s = b[(*p)++];
        if (s > max_sym) return BAD_FRAME;
        tab[0].sym = (uint8_t)s;
        tab[0].nbits = 0;
        tab[0].next = 0;
        *log = 0;
    } else {
        uint32_t nsym, used;
        int r = fse_read_norm(st, b + *p, bs - *p, max_log, max_sym, log, &nsym, &used);
        if (r) return r;
        r = fse_build(st, tab, *log, nsym);
        if (r) return r;
        *p += used;
    }
    *valid = 1;
    return OK;
}

// One compressed block b[0, bs): literals into lit (or taken in place), then the sequences, executed in batches.
template <class P>
PBSZ_HD int decode_block(State &st, const uint8_t *b, uint32_t bs, uint8_t *dst, uint32_t room, uint32_t &out, uint8_t *lit) {
    const bool lane0 = P::lane() == 0;
    const uint32_t block_out = out;
    (void)block_out;
    if (bs < 1) return BAD_FRAME;
    const uint32_t b0 = P::uni(b[0]), ltype = b0 & 3u, sf = (b0 >> 2) & 3u;
    uint32_t regen, comp = 0, lh, nstreams = 1;
    if (ltype < 2) {
        lh = sf == 1 ? 2u : sf == 3 ? 3u : 1u;
        if (bs < lh) return BAD_FRAME;
        regen = lh == 1 ? b0 >> 3 : (uint32_t)uload<P>(b, lh) >> 4;
        PBSZ_COV((ltype == 0 ? C_LIT_RAW_1 : C_LIT_RLE_1) + (int)lh - 1);
    } else {
        lh = sf < 2 ? 3u : sf + 2;
        if (bs < lh) return BAD_FRAME;
        const uint64_t v = uload<P>(b, lh);
        if (sf < 2) {
            regen = (uint32_t)(v >> 4) & 0x3ffu;
            comp = (uint32_t)(v >> 14) & 0x3ffu;
        } else if (sf == 2) {
            regen = (uint32_t)(v >> 4) & 0x3fffu;
            comp = (uint32_t)(v >> 18) & 0x3fffu;
        } else {
            regen = (uint32_t)(v >> 4) & 0x3ffffu;
            comp = (uint32_t)(v >> 22) & 0x3ffffu;
        }
        nstreams = sf == 0 ? 1u : 4u;
        PBSZ_COV(sf == 0 ? C_HUF_1STREAM : C_HUF_4STREAM_3 + (int)sf - 1);
    }
    if (regen > kLitMax) return BAD_FRAME;
    const uint8_t *litp = lit;
    uint32_t p;
    if (ltype == 0) {
        if (bs - lh < regen) return BAD_FRAME;
        litp = b + lh;
        p = lh + regen;
    } else if (ltype == 1) {
        if (bs - lh < 1) return BAD_FRAME;
        fill_bytes<P>(lit, (uint8_t)P::uni(b[lh]), regen);
        P::sync();
        p = lh + 1;
    } else {
        if (bs - lh < comp) return BAD_FRAME;
        const uint8_t *hp = b + lh;
        uint32_t used = 0;
        if (ltype == 2) {
            if (lane0) {
                uint32_t u = 0;
                st.err = huf_read_table(st, hp, comp, &u);
                st.tmp = u;
            }
            P::sync();
            if (P::uni((uint32_t)st.err)) return (int)P::uni((uint32_t)st.err);
            used = P::uni(st.tmp);
        } else {
            PBSZ_COV(C_HUF_TREELESS);
            if (!P::uni(st.huf_valid)) return BAD_FRAME;
        }
        const uint8_t *data = hp + used;
        const uint32_t dlen = comp - used;  // used <= comp: huf_read_table stays inside its bytes
        if (nstreams == 1) {
            if (lane0) {
                const int r = huf_stream(st, data, dlen, lit, regen);
                if (r) st.err = r;
            }
        } else {
            if (dlen < 6) return BAD_FRAME;
            const uint32_t c0 = (uint32_t)uload<P>(data, 2), c1 = (uint32_t)uload<P>(data + 2, 2), c2 = (uint32_t)uload<P>(data + 4, 2);
            if (dlen - 6 < c0 + c1 + c2) return BAD_FRAME;
            const uint32_t c3 = dlen - 6 - c0 - c1 - c2;
            const uint32_t seg = (regen + 3) / 4;
            if (3 * seg > regen) return BAD_FRAME;
            for (uint32_t s = (uint32_t)P::lane(); s < 4; s += (uint32_t)P::lanes()) {
                uint32_t so = 6, sl = c3;  // the stream's place from the jump table, read again by its own lane
                for (uint32_t j = 0; j < s; ++j) so += (uint32_t)load_le(data + 2 * j, 2);
                if (s < 3) sl = (uint32_t)load_le(data + 2 * s, 2);
                PBSZ_COV_IF(s == 3 && regen - 3 * seg < seg, C_HUF_SHORT_4TH);
                const int r = huf_stream(st, data + so, sl, lit + s * seg, s == 3 ? regen - 3 * seg : seg);
                if (r) st.err = r;
            }
        }
        P::sync();
        if (P::uni((uint32_t)st.err)) return (int)P::uni((uint32_t)st.err);
        p = lh + comp;
    }
    // the sequences section
    if (bs - p < 1) return BAD_FRAME;
    uint32_t nseq = P::uni(b[p++]);
    if (nseq == 0) {
        PBSZ_COV(C_NSEQ_0);
        if (p != bs) return BAD_FRAME;
    } else if (nseq < 128) {
        PBSZ_COV(C_NSEQ_1);
    } else if (nseq < 255) {
        if (bs - p < 1) return BAD_FRAME;
        nseq = ((nseq - 128) << 8) + P::uni(b[p++]);
        PBSZ_COV(C_NSEQ_2);
    } else {
        if (bs - p < 2) return BAD_FRAME;
        nseq = (uint32_t)uload<P>(b + p, 2) + 0x7f00u;
        p += 2;
        PBSZ_COV(C_NSEQ_3);
    }
    uint32_t litpos = 0;
    if (nseq) {
        if (bs - p < 1) return BAD_FRAME;
        const uint32_t modes = P::uni(b[p++]);
        if (lane0) {
            uint32_t q = p;
            int r = seq_table(st, 0, modes >> 6, b, bs, &q);
            if (!r) r = seq_table(st, 1, (modes >> 4) & 3u, b, bs, &q);
            if (!r) r = seq_table(st, 2, (modes >> 2) & 3u, b, bs, &q);
            st.err = r;
            st.tmp = q;
            st.out = out;
            st.litpos = 0;
        }
        P::sync();
        if (P::uni((uint32_t)st.err)) return (int)P::uni((uint32_t)st.err);
        p = P::uni(st.tmp);
        if (p >= bs) return BAD_FRAME;
        BitReader br;
        uint32_t s_ll = 0, s_of = 0, s_ml = 0;
        if (lane0) {
            if (!br.init(b + p, bs - p)) st.err = BAD_FRAME;
            s_ll = br.read(st.ll_log);
            s_of = br.read(st.of_log);
            s_ml = br.read(st.ml_log);
            if (br.over) st.err = BAD_FRAME;
        }
#ifdef PBSGPU_ZSTD_COVERAGE
        uint32_t prev_end = 0, prev_ml = 0;
#endif
        for (uint32_t done = 0; done < nseq;) {
            const uint32_t nb = nseq - done < (uint32_t)kBatch ? nseq - done : (uint32_t)kBatch;
            if (lane0 && !st.err) {  // the serial chain: states, extra bits, repeat offsets, and every bound
                uint32_t o = st.out;
                uint32_t lp = st.litpos;
                int err = OK;
                for (uint32_t k = 0; k < nb; ++k) {
                    const FseEntry e_ll = st.ll[s_ll], e_of = st.of[s_of], e_ml = st.ml[s_ml];
                    const uint32_t ofc = e_of.sym;  // <= 31 by construction of the table
                    const uint32_t ov = (1u << ofc) + br.read(ofc);
                    const uint32_t ml = kMLBase[e_ml.sym] + br.read(kMLBits[e_ml.sym]);
                    const uint32_t ll = kLLBase[e_ll.sym] + br.read(kLLBits[e_ll.sym]);
                    uint32_t off;
                    if (ov > 3) {
                        off = ov - 3;
                        st.rep[2] = st.rep[1];
                        st.rep[1] = st.rep[0];
                        st.rep[0] = off;
                    } else {
                        const uint32_t idx = ov + (ll == 0 ? 1u : 0u);  // 1..4
                        if (ll == 0) PBSZ_COV(C_REP_SHIFTED);
                        if (idx == 1) {
                            PBSZ_COV(C_REP_1);
                            off = st.rep[0];
                        } else {
                            if (idx == 4) PBSZ_COV(C_REP_1_MINUS_1);
                            else PBSZ_COV(idx == 2 ? C_REP_2 : C_REP_3);
                            off = idx == 2 ? st.rep[1] : idx == 3 ? st.rep[2] : st.rep[0] - 1;
                            if (idx != 2) st.rep[2] = st.rep[1];
                            st.rep[1] = st.rep[0];
                            st.rep[0] = off;
                        }
                    }
                    if (done + k + 1 < nseq) {
                        s_ll = e_ll.next + br.read(e_ll.nbits);
                        s_ml = e_ml.next + br.read(e_ml.nbits);
                        s_of = e_of.next + br.read(e_of.nbits);
                    }
                    if (br.over || ll > regen - lp || off == 0 || off > (uint64_t)o + ll) {
                        err = BAD_FRAME;
                        break;
                    }
                    if ((uint64_t)ll + ml > room - o) {
                        err = BAD_SIZE;
                        break;
                    }
                    if (off < ml) PBSZ_COV(C_MATCH_OVERLAP);
                    if (off == 1) PBSZ_COV(C_MATCH_OFFSET_1);
                    if (off > o + ll - block_out) PBSZ_COV(C_MATCH_ACROSS_BLOCKS);
                    st.seq[k].out = o;
                    st.seq[k].lit = lp;
                    st.seq[k].ll = ll;
                    st.seq[k].ml = ml;
                    st.seq[k].off = off;
                    lp += ll;
                    o += ll + ml;
                }
                st.err = err;
                st.out = o;
                st.litpos = lp;
            }
            P::sync();
            if (P::uni((uint32_t)st.err)) return (int)P::uni((uint32_t)st.err);
            // literal runs: short ones one lane each, long ones by all lanes
            for (uint32_t k = (uint32_t)P::lane(); k < nb; k += (uint32_t)P::lanes()) {
                const uint32_t ll = st.seq[k].ll;
                PBSZ_COV_IF(ll > 0 && ll <= 16, C_LIT_SHORT);
                PBSZ_COV_IF(ll > 16, C_LIT_LONG);
                if (ll <= 16) {
                    uint8_t *d = dst + st.seq[k].out;
                    const uint8_t *s = litp + st.seq[k].lit;
                    for (uint32_t i = 0; i < ll; ++i) d[i] = s[i];
                }
            }
            for (uint32_t k = 0; k < nb; ++k)
                if (P::uni(st.seq[k].ll) > 16) copy_bytes<P>(dst + P::uni(st.seq[k].out), litp + P::uni(st.seq[k].lit), P::uni(st.seq[k].ll));
            P::sync();
            // matches in order, each by all lanes. `seen` = the output position below which every byte is known to be
            // visible to every lane; a match whose source reaches past it waits for the stores before it.
            uint32_t seen = P::uni(st.seq[0].out + st.seq[0].ll);
            for (uint32_t k = 0; k < nb; ++k) {
                const uint32_t at = P::uni(st.seq[k].out + st.seq[k].ll);
                const uint32_t ml = P::uni(st.seq[k].ml), off = P::uni(st.seq[k].off);
                const uint32_t span = off < ml ? off : ml;
                PBSZ_COV_IF(at - off + span > seen, C_MATCH_WAIT);
                PBSZ_COV_IF(at - off + span <= seen, C_MATCH_NO_WAIT);
                PBSZ_COV_IF(st.seq[k].ll > 0 && at - off + span > st.seq[k].out, C_MATCH_SRC_OWN_LITERALS);
                // (prev_end: where the match before this one ended, in this batch or the one before; 0 = none in this block)
                PBSZ_COV_IF(k > 0 && at - off < prev_end && at - off + span > prev_end - prev_ml, C_MATCH_SRC_IN_PREV_MATCH);
                PBSZ_COV_IF(k == 0 && done > 0 && at - off < prev_end && at - off + span > prev_end - prev_ml, C_BATCH_FOLLOWS_BATCH);
                if (at - off + span > seen) {
                    P::sync();
                    seen = at;
                }
#ifdef PBSGPU_ZSTD_COVERAGE
                prev_end = at + ml;
                prev_ml = ml;
#endif
                uint8_t *d = dst + at;
                const uint8_t *s = d - off;
                if (off >= ml)
                    for (uint32_t i = (uint32_t)P::lane(); i < ml; i += (uint32_t)P::lanes()) d[i] = s[i];
                else
                    for (uint32_t i = (uint32_t)P::lane(); i < ml; i += (uint32_t)P::lanes()) d[i] = s[i % off];
            }
            done += nb;
            P::sync();  // the batch is free for lane 0 again
        }
        out = P::uni(st.out);
        litpos = P::uni(st.litpos);
    }
    const uint32_t tail = regen - litpos;  // literals after the last sequence
    if (tail > room - out) return BAD_SIZE;
    copy_bytes<P>(dst + out, litp + litpos, tail);
    out += tail;
    return OK;
}

// What a decoded frame says of itself beyond its bytes: for a caller that walks a stream or verifies the checksum
// (zstd_stream.h). decode_frame drops it.
struct FrameEnd {
    uint32_t used;          // the frame's own bytes, header to checksum; 0: the decoder did not get that far
    uint32_t has_checksum;
    uint32_t checksum;      // the stored low word of XXH64(content, 0)
};

// Decodes the frame that starts at src[0] into dst[0, room): n = the bytes that may be read, both below 4 GiB (a chunk is
// 16 MiB at the most). kAlone: the frame must end at src + n, anything behind it is UNSUPPORTED (a blob is one frame);
// otherwise the caller goes on at src + end.used, or decides itself that bytes are left over: end.used is set, with any
// status, once the frame's last byte has been found, and 0 before. lit: kLitMax bytes of scratch for this call. *decoded = bytes produced
// and `end` (both valid with OK). Never loads outside src[0, n), never stores outside dst[0, room) and lit[0, kLitMax).
template <class P, bool kAlone>
PBSZ_HD int decode_frame_at(State &st, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t room, uint8_t *lit,
                            uint32_t *decoded, FrameEnd &end) {
    *decoded = 0;
    end.used = end.has_checksum = end.checksum = 0;
    FrameHeader h;
    const int r = parse_frame_header<P>(src, n, h);
    if (r) return r;
    if (h.content_size != kNoSize && h.content_size > room) return BAD_SIZE;
    const bool sized = h.content_size != kNoSize;
    const uint32_t want = (uint32_t)h.content_size, has_checksum = h.has_checksum;
    if (P::lane() == 0) {
        st.err = 0;
        st.huf_valid = st.ll_valid = st.of_valid = st.ml_valid = 0;
        st.rep[0] = 1;
        st.rep[1] = 4;
        st.rep[2] = 8;
    }
    P::sync();
    uint32_t pos = h.header_bytes, out = 0;
    for (uint32_t nblocks = 0;; ++nblocks) {
        (void)nblocks;
        if (n - pos < 3) return BAD_FRAME;
        const uint32_t bh = (uint32_t)uload<P>(src + pos, 3);
        pos += 3;
        const uint32_t last = bh & 1u, type = (bh >> 1) & 3u, bsize = bh >> 3;
        if (bsize > kBlockMax) return BAD_FRAME;  // Block_Maximum_Size, for raw and RLE blocks too
        if (nblocks > 0) PBSZ_COV(C_MANY_BLOCKS);
        if (nblocks > 0 && last && bsize == 0 && type == 0) PBSZ_COV(C_EMPTY_LAST_BLOCK);
        if (type == 0) {
            PBSZ_COV(C_BLOCK_RAW);
            if (n - pos < bsize) return BAD_FRAME;
            if (room - out < bsize) return BAD_SIZE;
            copy_bytes<P>(dst + out, src + pos, bsize);
            pos += bsize;
            out += bsize;
        } else if (type == 1) {
            PBSZ_COV(C_BLOCK_RLE);
            if (n - pos < 1) return BAD_FRAME;
            if (room - out < bsize) return BAD_SIZE;
            fill_bytes<P>(dst + out, (uint8_t)P::uni(src[pos]), bsize);
            pos += 1;
            out += bsize;
        } else if (type == 2) {
            PBSZ_COV(C_BLOCK_COMPRESSED);
            if (n - pos < bsize) return BAD_FRAME;
            const int rb = decode_block<P>(st, src + pos, bsize, dst, room, out, lit);
            if (rb) return rb;
            pos += bsize;
        } else {
            return BAD_FRAME;
        }
        P::sync();  // the next block may match into this one, and reuses lit
        if (last) break;
    }
    if (has_checksum) {  // XXH64 low word: accounted for here, verified by the caller that was asked to (zstd_stream.h)
        if (n - pos < 4) return BAD_FRAME;
        end.checksum = (uint32_t)load_le(src + pos, 4);  // (a plain load: dropped where `end` is)
        pos += 4;
    }
    end.used = pos;
    end.has_checksum = has_checksum;
    if (kAlone && pos != n) return UNSUPPORTED;  // a second frame, a skippable frame, or garbage behind the frame
    if (sized && want != out) return BAD_SIZE;
    *decoded = out;
    return OK;
}

// Decodes the one frame src[0, n): the restore's call (k_zstd_frames) and pbsgpu_zstd_decode_device.
template <class P>
PBSZ_HD int decode_frame(State &st, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t room, uint8_t *lit,
                         uint32_t *decoded) {
    FrameEnd end;
    return decode_frame_at<P, true>(st, src, n, dst, room, lit, decoded, end);
}


}  // namespace pbsz
