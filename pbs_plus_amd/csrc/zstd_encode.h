// Zstandard frame encoding (RFC 8878) for the write side: ONE implementation, compiled twice, in the manner of
// zstd_decode.h, whose tables, constants and FSE table build it uses. Under hipcc every function is __host__ __device__ and
// zstd_encode.hip runs encode_block with one wave per 128 KiB block; without hipcc it is plain inline C++, and that build
// is what tests/native/test_zstd_encode.cpp runs under AddressSanitizer. No HIP and no libc.
//
// The policy P is the decoder's (lane, lanes, sync, uni) plus the two read-modify-writes that lanes aim at one word:
//   P::amax(p, v)  *p = max(*p, v), atomically among the lanes
//   P::aadd(p, v)  *p += v, atomically among the lanes
// Every phase is `for (l = P::lane(); l < 64; l += P::lanes())` between P::sync()s, so one host lane does exactly what 64
// device lanes do and both builds write the same bytes (tests/golden/zstd_enc_v1.json).
//
// Decisions (include/pbsgpu.h):
//   * Frame: magic, single segment, no dictionary id, no checksum; the content size in 1, 2 or 4 bytes. Blocks carry
//     kBlockMax = 128 KiB of content each; 0 bytes of content is a header and one empty raw last block.
//   * Blocks are independent: a match never reaches before its block's first byte. Repeats further apart are not found.
//   * A block of one byte value is an RLE block; a block whose compressed form is not smaller than its content is raw.
//   * Match finder: greedy, minimum match 4. hash[h] = 1 + the highest block-relative position inserted with hash h.
//     Positions are worked in batches of 64: every position looks the table up as it stood before the batch, verifies and
//     extends its candidate up to the block's end; then the batch inserts itself (amax); lane 0 takes the matches in
//     position order, the first one at or after the cursor, and the cursor moves to that match's end.
//     A batch starts at the cursor or behind the batch before it, whichever is later: every position of a batch is
//     inserted, whether a taken match covers it or not, and the positions a taken match carries the cursor over beyond its
//     batch are neither looked up nor inserted.
//   * Sequences: Predefined_Mode for all three symbol types, only offset + 3 values (no repeat codes, so no history). At
//     most kSeqCap per block; behind the cap the block's remaining bytes are literals. kSeqCap < 0x7F00: the 3-byte count
//     form never occurs. Lane 0 encodes them in reverse into the backward bit stream.
//   * Literals: histogram by all lanes, the length-limited (kHufMaxBits = 11) code by lane 0, one stream up to 1 023
//     literals and four streams on lanes 0-3 above. Huffman only if the tree description plus the streams is strictly
//     smaller than the literals; one byte value is RLE literals; no literals or no gain is raw literals.
//     The weights are described directly (highest byte value <= 128) or FSE-compressed, whichever is smaller and fits the
//     header byte; where neither does, the literals stay raw ("Huffman refused").
//   * The encoder knows its room and writes nothing outside it; a room below what the frame needs is BAD_SIZE.
//   * A second way to write the sequences (TState instead of State; pbsgpu_engine_options::zstd_seq_tables = 1): the same
//     sequences, with repeat codes and per-block tables. The match finder, the literals and every other rule are the above.
//     - Repeat codes against a history that starts UNKNOWN in every block, because the decoder's history comes from the
//       blocks before and a block's encoder does not know them: an explicit offset makes entry 0 known and shifts values
//       and known flags as the decoder shifts; a repeat code is written only for a known entry that equals the offset,
//       and its rotation moves the flags too. Lane 0 converts where it takes the matches; bits 53-54 of the word.
//     - Per symbol type Predefined_Mode, RLE_Mode (one code occurs) or FSE_Compressed_Mode, never Repeat_Mode. The
//       accuracy log is highbit(nseq - 1) - 2 within [5, 9 / 8 / 9], raised until every occurring code has a state; the
//       counts are scaled to 1 << log with rounding, at least 1 each, and the difference goes to (or comes off) the most
//       frequent code; "less than 1" probabilities are not used (such a code gets one state either way). The choice is
//       by count * (log - log2 p) in 1/256 bit plus the description's bytes, integers on both builds; RLE and compressed
//       must beat predefined by kSeqMargin bits, which covers what the estimate can be off by, so that a frame of this
//       mode is never longer than the other mode's.
//   * A long-range variant of the match finder (WState / WTState instead of State / TState;
//     pbsgpu_engine_options::zstd_window_log = 17, 18 or 19), chosen at compile time:
//     - a block's matches may start in its HISTORY, the hn = min(block's place in the chunk, 1 << window_log) bytes of the
//       chunk in front of it. All of a chunk's content is there before its first block is encoded, so the blocks stay
//       independent of each other's ENCODING, and the frame is single-segment: any offset up to the position is valid.
//     - the table has 1 << kWindowHashLog entries and is the caller's, reached through a pointer; an entry is 1 + the
//       highest WINDOW-relative position inserted (position 0 is the first history byte). Behind the RLE test every
//       history position whose four bytes end inside the block's end is inserted; then the batches run as above, from the
//       block's first byte. A match may start in the history and run into the block; its length is bounded by the
//       block's end and its offset is the distance in the chunk. A chunk of one block uses this table too.
//     - the content is read through a source type C (at, rd32, from): a plain pointer, or Src2 for a chunk in two parts.
//     - offsets reach (1 << 19) + kBlockMax: the word is 18 | 18 | 20 bits with the repeat code in bits 56-57, and offset
//       codes go up to 19 (the predefined distribution has a state for every code to 28). Repeat offsets as above.
//     - a frame of this mode may be a little LONGER than the other match finder's on content without far repeats.
//   * Buffers a block needs, all implied by kBlockMax: lit kBlockMax bytes, seqs kSeqCap * 8 bytes, blk kBlockMax bytes (a
//     compressed form that would pass the block's content length is abandoned where it would).
#pragma once

#include "xxh64.h"
#include "zstd_decode.h"

#ifdef PBSGPU_ZSTD_COVERAGE  // CPU test build only: one bit per branch (names: tests/test_zstd_encode_native.py)
namespace pbsz {
namespace enc {
inline uint64_t g_cov = 0;
}
}
#define PBSZ_ECOV(bit) (::pbsz::enc::g_cov |= 1ull << (bit))
#else
#define PBSZ_ECOV(bit) ((void)0)
#endif

namespace pbsz {
namespace enc {

enum : int {  // coverage bits
    E_FCS_1, E_FCS_2, E_FCS_4, E_BLOCK_RAW, E_BLOCK_RLE, E_BLOCK_COMPRESSED, E_EMPTY_LAST_BLOCK,
    E_LIT_RAW, E_LIT_RLE, E_HUF_1STREAM, E_HUF_4STREAM, E_WEIGHTS_DIRECT, E_WEIGHTS_FSE,
    E_NSEQ_0, E_NSEQ_1, E_NSEQ_2, E_MATCH_OVERLAP, E_MATCH_OFFSET_1, E_LL_EXTRA, E_ML_EXTRA, E_SEQ_CAP, E_HUF_REFUSED,
    E_NBITS
};
enum : int {  // ... of the mode with tables and repeat codes alone: the mode of each type (predefined, RLE, compressed; LL, OF,
              // ML), the repeat codes behind literals and behind none, a repeat the decoder could have taken whose entry
              // this block does not know, the longest accuracy log of each type
    E_LL_PREDEF = E_NBITS, E_LL_RLE, E_LL_FSE, E_OF_PREDEF, E_OF_RLE, E_OF_FSE, E_ML_PREDEF, E_ML_RLE, E_ML_FSE,
    E_REP_1, E_REP_2, E_REP_3, E_REP0_1, E_REP0_2, E_REP0_3, E_REP_UNKNOWN, E_LL_LOG_MAX, E_OF_LOG_MAX, E_ML_LOG_MAX,
    E_NBITS_TABLES
};
enum : int {  // ... of the long-range match finder alone: a candidate in the history, a match that starts in the history and
              // runs into the block, a history that the window cuts (what lies before it is not inserted, so a match
              // there is refused), an offset code of 18 or 19, a history that the chunk's start cuts
    E_W_CAND_HISTORY = E_NBITS_TABLES, E_W_CROSS, E_W_BEYOND, E_W_OF_18, E_W_CHUNK_START,
    E_NBITS_WINDOW
};

constexpr uint32_t kHashLog = 12;
constexpr uint32_t kWindowHashLog = 14;  // the long-range match finder's table, in the caller's memory
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kLanes = 64;           // a batch of positions
constexpr uint32_t kSeqCap = 24576;       // sequences per block; 8 bytes each in the caller's scratch
constexpr uint32_t kHufMaxBits = 11;
constexpr uint32_t kNone = 0xffffffffu;
enum : uint32_t { B_RAW = 0, B_RLE = 1, B_COMPRESSED = 2 };

struct HostLanes : pbsz::HostLanes {
    static PBSZ_HD void amax(uint32_t *p, uint32_t v) {
        if (*p < v) *p = v;
    }
    static PBSZ_HD void aadd(uint32_t *p, uint32_t v) { *p += v; }
};

struct EncTab {  // FSE encoding of one predefined distribution, derived from the decoding table fse_build makes
    typedef uint8_t state_t;
    uint8_t state[64];  // state[cum[s] + k]: the k-th state (ascending) that decodes to s
    uint8_t cum[53], p[53];
    uint32_t log;
};

// Per block in flight; LDS in the kernel. The decoder's State is needed only while FSE tables are built (the predefined
// ones before the first block, the weights' own after a block's match finding): it shares its bytes with the hash table.
struct State {
    static constexpr bool kSeqTables = false;
    static constexpr bool kWindow = false;
    union {
        uint32_t hash[1u << kHashLog];
        pbsz::State dec;
    } u;
    uint32_t hist[256];   // literal counts
    uint32_t key[256];    // the counts in ascending order, then the code lengths (in place)
    uint16_t code[256];
    uint8_t len[256];     // 0: the byte value does not occur
    uint8_t sorted[256];  // byte values by ascending (count, value)
    EncTab ll, of, ml, wt;  // wt: the weights' own distribution, per block
    uint8_t wdesc[128];     // the FSE-compressed weight description, header byte first
    uint32_t mlen[kLanes], moff[kLanes], mh[kLanes], lidx[kLanes];  // the batch
    uint32_t ncodes[40], start[kHufMaxBits + 2];
    uint32_t sbits[4];
    uint32_t flag, cursor, nlit, nseq, ll_run, next_b0;
    uint32_t nsym, maxsym, maxcnt, maxbits, desc, wfse, size, over;
};

// The mode with per-block sequence tables and repeat codes: State and what that mode adds. enc::State itself stays as it
// is, and with it the kernel of the other mode.
struct SeqTab {  // FSE encoding of one block's distribution of one symbol type: up to 512 states, probabilities up to 512
    typedef uint16_t state_t;
    uint16_t state[512];
    uint16_t cum[53], p[53];
    uint32_t log;  // 0: RLE_Mode, one state that takes no bits
};
constexpr uint32_t kSeqDescMax = 80;  // an NCount stream: 4 bits, then at most 10 bits and a 2-bit zero run per code: 4 + 53 * 12 bits
constexpr uint32_t kSeqMargin = 16;   // bits, plus nseq / 64 (see choose_table)
struct TState : State {
    static constexpr bool kSeqTables = true;
    SeqTab tab[3];                  // LL, OF, ML
    uint32_t shist[3][64];          // the counts of the three code streams
    uint8_t sdesc[3][kSeqDescMax];  // RLE_Mode: the code; FSE_Compressed_Mode: the NCount stream
    uint32_t smode[3], sdlen[3];
    uint32_t rep[3], known;         // the block's own offset history; known: bit i says that rep[i] is what the decoder has
};

// The long-range match finder on either way to write the sequences: the same bytes in LDS (u.hash serves only as the
// decoder's State while tables are built), another type for encode_block to choose by.
struct WState : State {
    static constexpr bool kWindow = true;
};
struct WTState : TState {
    static constexpr bool kWindow = true;
};
// the sequence word: literal length | match length << 18 | offset << 36 | repeat code << rep_shift
template <class S> constexpr uint32_t off_mask = S::kWindow ? 0xfffffu : 0x1ffffu;
template <class S> constexpr uint32_t rep_shift = S::kWindow ? 56u : 53u;

// Content in two parts (a ring chunk in two pages): byte i is p0[i] below a and p1[i - a] from a on. One part: a = its length.
struct Src2 {
    const uint8_t *p0, *p1;
    uint32_t a;
};

#ifdef PBSGPU_ZSTD_COVERAGE  // CPU test build only: the history the decoder really has, for E_REP_UNKNOWN alone
inline uint32_t g_dec_rep[3] = {1, 4, 8}, g_dec_rep_block[3] = {1, 4, 8};
#endif

PBSZ_HD uint32_t header_bytes(uint64_t n) { return 5u + (n <= 255 ? 1u : n <= 65791 ? 2u : 4u); }
PBSZ_HD uint64_t block_count(uint64_t n) { return n ? (n + kBlockMax - 1) / kBlockMax : 1; }
// no frame of n bytes of content is longer: the header, three bytes per block, the content
PBSZ_HD uint64_t encode_bound(uint64_t n) { return header_bytes(n) + 3 * block_count(n) + n; }

// ... and with a content checksum: the low word of XXH64(content, 0) behind the last block
PBSZ_HD uint64_t encode_bound2(uint64_t n, bool checksum) { return encode_bound(n) + (checksum ? 4u : 0u); }

// the frame header of n < 4 GiB bytes of content into h[0, header_bytes(n)); checksum: Content_Checksum_flag
PBSZ_HD void frame_header(uint64_t n, uint8_t *h, bool checksum = false) {
    const uint32_t hb = header_bytes(n), fcs = hb - 5;
    h[0] = 0x28;
    h[1] = 0xb5;
    h[2] = 0x2f;
    h[3] = 0xfd;
    h[4] = (uint8_t)((fcs == 1 ? 0u : fcs == 2 ? 1u : 2u) << 6 | 1u << 5 | (checksum ? 1u << 2 : 0u));
    const uint64_t v = fcs == 2 ? n - 256 : n;
    for (uint32_t i = 0; i < fcs; ++i) h[5 + i] = (uint8_t)(v >> (8 * i));
    PBSZ_ECOV(fcs == 1 ? E_FCS_1 : fcs == 2 ? E_FCS_2 : E_FCS_4);
}

// a block's three header bytes; bytes = the block's content length for raw and RLE, the compressed size otherwise
PBSZ_HD void block_header(uint8_t *h, uint32_t last, uint32_t type, uint32_t bytes) {
    const uint32_t v = last | type << 1 | bytes << 3;
    h[0] = (uint8_t)v;
    h[1] = (uint8_t)(v >> 8);
    h[2] = (uint8_t)(v >> 16);
}
// the bytes behind the header: the content, one byte, the compressed form
PBSZ_HD uint32_t payload_bytes(uint32_t type, uint32_t bn, uint32_t csize) { return type == B_RAW ? bn : type == B_RLE ? 1u : csize; }

PBSZ_HD uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
PBSZ_HD uint32_t hash4(uint32_t v, uint32_t log = kHashLog) { return (v * 2654435761u) >> (32 - log); }
// a source C: the byte and the four bytes at i, or at i + k (two steps, so that the pointer form is the expression it
// always was), and the source k bytes further on
PBSZ_HD uint8_t at(const uint8_t *s, uint32_t i) { return s[i]; }
template <class T>
PBSZ_HD uint8_t at(const uint8_t *s, uint32_t i, T k) { return s[i + k]; }
PBSZ_HD uint32_t rd32(const uint8_t *s, uint32_t i) { return rd32(s + i); }
template <class T>
PBSZ_HD uint32_t rd32(const uint8_t *s, uint32_t i, T k) { return rd32(s + i + k); }
PBSZ_HD const uint8_t *from(const uint8_t *s, uint32_t k) { return s + k; }
PBSZ_HD uint8_t at(const Src2 &s, uint32_t i) { return i < s.a ? s.p0[i] : s.p1[i - s.a]; }
PBSZ_HD uint32_t rd32(const Src2 &s, uint32_t i) {
    if (i + 4 <= s.a) return rd32(s.p0 + i);
    if (i >= s.a) return rd32(s.p1 + (i - s.a));
    return (uint32_t)at(s, i) | (uint32_t)at(s, i + 1) << 8 | (uint32_t)at(s, i + 2) << 16 | (uint32_t)at(s, i + 3) << 24;
}
template <class T>
PBSZ_HD uint8_t at(const Src2 &s, uint32_t i, T k) { return at(s, i + (uint32_t)k); }
template <class T>
PBSZ_HD uint32_t rd32(const Src2 &s, uint32_t i, T k) { return rd32(s, i + (uint32_t)k); }
PBSZ_HD Src2 from(const Src2 &s, uint32_t k) {
    if (k < s.a) return Src2{s.p0 + k, s.p1, s.a - k};
    return Src2{s.p1 + (k - s.a), s.p1 + (k - s.a), 0};
}

// A backward bit stream being written: values go in from bit 0 of p[0] upwards, the reader takes them from the top. No byte
// at or behind p[cap] is stored; `over` says that one would have been.
struct BitWriter {
    uint8_t *p;
    uint32_t pos, cap, nb;
    uint64_t acc;
    bool over;

    PBSZ_HD void init(uint8_t *dst, uint32_t room) {
        p = dst;
        pos = 0;
        cap = room;
        nb = 0;
        acc = 0;
        over = false;
    }
    PBSZ_HD void put_byte() {
        if (pos < cap) p[pos] = (uint8_t)acc;
        else over = true;
        ++pos;
        acc >>= 8;
    }
    PBSZ_HD void add(uint32_t v, uint32_t k) {  // v < 1 << k, k <= 32
        acc |= (uint64_t)v << nb;
        nb += k;
        while (nb >= 8) {
            put_byte();
            nb -= 8;
        }
    }
    PBSZ_HD uint32_t flush() {  // a forward stream's last partial byte; returns the length
        if (nb) {
            put_byte();
            nb = 0;
        }
        return pos;
    }
    PBSZ_HD uint32_t finish() {  // the end mark; returns the stream's length
        add(1, 1);
        if (nb) {
            put_byte();
            nb = 0;
        }
        return pos;
    }
};

// t.state from t.cum, t.p, t.log and the decoding table: a state's rank among those of its symbol is what its baseline says
template <class T>
PBSZ_HD void rank_states(T &t, const FseEntry *tab) {
    const uint32_t size = 1u << t.log;
    PBSZ_ROLLED
    for (uint32_t u = 0; u < size; ++u) {
        const uint32_t s = tab[u].sym;
        t.state[t.cum[s] + ((tab[u].next + size) >> tab[u].nbits) - t.p[s]] = (typename T::state_t)u;
    }
}

// The three predefined encoding tables (lane 0, once before the first block; the hash table's bytes serve as the decoder
// state that fse_build works in).
PBSZ_HD void build_tab(State &st, uint32_t which) {
    EncTab &t = which == 0 ? st.ll : which == 1 ? st.of : st.ml;
    uint32_t q = 0;
    (void)seq_table(st.u.dec, which, 0, nullptr, 0, &q);  // the predefined distribution: cannot fail
    const FseEntry *tab = which == 0 ? st.u.dec.ll : which == 1 ? st.u.dec.of : st.u.dec.ml;
    const uint32_t n = which == 0 ? 36u : which == 1 ? 29u : 53u;
    t.log = which == 1 ? 5u : 6u;
    uint32_t cum = 0;
    PBSZ_ROLLED
    for (uint32_t s = 0; s < n; ++s) {
        const int32_t v = which == 0 ? kLLDefault[s] : which == 1 ? kOFDefault[s] : kMLDefault[s];
        const uint32_t p = v < 0 ? 1u : (uint32_t)v;
        t.p[s] = (uint8_t)p;
        t.cum[s] = (uint8_t)cum;
        cum += p;
    }
    rank_states(t, tab);
}

template <class P>
PBSZ_HD void init_tables(State &st) {
    if (P::lane() == 0) {
        build_tab(st, 0);
        build_tab(st, 1);
        build_tab(st, 2);
    }
    P::sync();
}

// symbol s goes in front of what state X stands for: the bits the decoder reads to get from s's state to X
template <class T>
PBSZ_HD void fse_put(const T &t, uint32_t &X, uint32_t s, BitWriter &bw) {
    const uint32_t x = X + (1u << t.log), p = t.p[s];
    uint32_t nb = t.log - highbit(p);
    if ((x >> nb) < p) --nb;
    bw.add(x & ((1u << nb) - 1), nb);
    X = t.state[t.cum[s] + (x >> nb) - p];
}

PBSZ_HD uint32_t ll_code(uint32_t ll) {
    if (ll < 16) return ll;
    if (ll >= 64) return highbit(ll) + 19;
    uint32_t c = 16;
    PBSZ_ROLLED
    while (kLLBase[c + 1] <= ll) ++c;  // ends at 24 at the latest: kLLBase[25] = 64
    return c;
}

PBSZ_HD uint32_t ml_code(uint32_t ml) {  // ml >= 3
    const uint32_t b = ml - 3;
    if (b < 32) return b;
    if (b >= 128) return highbit(b) + 36;
    uint32_t c = 32;
    PBSZ_ROLLED
    while (kMLBase[c + 1] <= ml) ++c;  // ends at 42 at the latest: kMLBase[43] = 131
    return c;
}

// Code lengths of minimum redundancy, in place (Moffat and Katajainen): A[0, n) are the counts in ascending order on entry
// and the code lengths, longest first, on return. n >= 2.
PBSZ_HD void min_redundancy(uint32_t *A, int32_t n) {
    A[0] += A[1];
    int32_t root = 0, leaf = 2, next;
    for (next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) {
            A[next] = A[root];
            A[root++] = (uint32_t)next;
        } else {
            A[next] = A[leaf++];
        }
        if (leaf >= n || (root < next && A[root] < A[leaf])) {
            A[next] += A[root];
            A[root++] = (uint32_t)next;
        } else {
            A[next] += A[leaf++];
        }
    }
    A[n - 2] = 0;
    for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int32_t avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int32_t)A[root] == dpth) {
            ++used;
            --root;
        }
        while (avbl > used) {
            A[next--] = (uint32_t)dpth;
            --avbl;
        }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
}

// Lane 0: from st.sorted / st.key (nsym >= 2 byte values by ascending count) the code lengths of at most kHufMaxBits and
// the codes as the decoder's table has them (weight 1 first, byte values ascending within a weight); st.maxbits.
PBSZ_HD void huf_build(State &st, uint32_t nsym) {
    min_redundancy(st.key, (int32_t)nsym);
    PBSZ_ROLLED
    for (uint32_t i = 0; i < 40; ++i) st.ncodes[i] = 0;
    for (uint32_t i = 0; i < nsym; ++i) st.ncodes[st.key[i] < 39 ? st.key[i] : 39]++;
    // the length limit: every longer code becomes kHufMaxBits long, then the Kraft sum is brought back to one
    for (uint32_t i = kHufMaxBits + 1; i < 40; ++i) st.ncodes[kHufMaxBits] += st.ncodes[i];
    uint32_t total = 0;
    for (uint32_t i = kHufMaxBits; i > 0; --i) total += st.ncodes[i] << (kHufMaxBits - i);
    while (total != (1u << kHufMaxBits)) {
        st.ncodes[kHufMaxBits]--;
        for (uint32_t i = kHufMaxBits - 1; i > 0; --i)
            if (st.ncodes[i]) {
                st.ncodes[i]--;
                st.ncodes[i + 1] += 2;
                break;
            }
        --total;
    }
    uint32_t j = nsym, maxbits = 0;
    for (uint32_t i = 1; i <= kHufMaxBits; ++i) {
        if (st.ncodes[i]) maxbits = i;
        for (uint32_t l = st.ncodes[i]; l > 0; --l) st.len[st.sorted[--j]] = (uint8_t)i;
    }
    st.maxbits = maxbits;
    uint32_t at = 0;  // first table index of each weight w = maxbits + 1 - length
    for (uint32_t w = 1; w <= maxbits; ++w) {
        st.start[w] = at;
        at += st.ncodes[maxbits + 1 - w] << (w - 1);
    }
    PBSZ_ROLLED
    for (uint32_t s = 0; s < 256; ++s) {
        const uint32_t l = st.len[s];
        if (!l) continue;
        const uint32_t w = maxbits + 1 - l;
        st.code[s] = (uint16_t)(st.start[w] >> (w - 1));
        st.start[w] += 1u << (w - 1);
    }
}

// Lane 0, after huf_build: the FSE-compressed description of the weights of byte values 0 .. maxsym - 1 into st.wdesc,
// header byte first. Returns its length, or 0 where there is none: fewer than two weights, one weight value only (its
// states would take no bits and the decoder could not find the end), or more than 127 bytes. The distribution is brought
// to 64 (accuracy log 6, the most a weight description may have) by rounding down, at least 1 for a value that occurs,
// and the difference goes to the most frequent value. Works in the decoder state that shares the hash table's bytes.
PBSZ_HD uint32_t weights_fse(State &st, uint32_t maxsym) {
    pbsz::State &d = st.u.dec;
    const uint32_t maxbits = st.maxbits, nw = maxsym, log = 6;
    if (nw < 2) return 0;
    PBSZ_ROLLED
    for (uint32_t w = 0; w < kHufLogMax + 2; ++w) d.rank[w] = 0;
    PBSZ_ROLLED
    for (uint32_t i = 0; i < nw; ++i) {
        const uint32_t l = st.len[i], w = l ? maxbits + 1 - l : 0u;
        d.weights[i] = (uint8_t)w;
        d.rank[w]++;
    }
    uint32_t nsym = 0, distinct = 0, sum = 0, big = 0;
    PBSZ_ROLLED
    for (uint32_t w = 0; w <= maxbits; ++w) {
        const uint32_t c = d.rank[w];
        uint32_t p = 0;
        if (c) {
            nsym = w + 1;
            ++distinct;
            p = (c << log) / nw;
            if (!p) p = 1;
        }
        d.norm[w] = (int16_t)p;
        sum += p;
        if (p > (uint32_t)d.norm[big]) big = w;
    }
    if (distinct < 2) return 0;
    while (sum > (1u << log)) {  // (rounding up to 1 overshot: at most eleven steps, and a value above 1 exists)
        PBSZ_ROLLED
        for (uint32_t w = 0; w < nsym; ++w)
            if (d.norm[w] > d.norm[big]) big = w;
        d.norm[big]--;
        --sum;
    }
    d.norm[big] = (int16_t)(d.norm[big] + (int32_t)((1u << log) - sum));
    BitWriter bw;
    bw.init(st.wdesc + 1, 127);
    bw.add(log - 5, 4);
    uint32_t remaining = 1u << log, s = 0;
    while (remaining > 0 && s < nsym) {  // fse_read_norm, the other way round
        const uint32_t R = remaining + 1, bits = highbit(R) + 1, lower = (1u << (bits - 1)) - 1, thr = (1u << bits) - 1 - R;
        const uint32_t p = (uint32_t)d.norm[s++], val = p + 1;
        if (val < thr) bw.add(val, bits - 1);
        else bw.add(val > lower ? val + thr : val, bits);
        remaining -= p;
        if (p == 0) {
            uint32_t z = 0;
            while (s < nsym && d.norm[s] == 0) {
                ++z;
                ++s;
            }
            while (z >= 3) {
                bw.add(3, 2);
                z -= 3;
            }
            bw.add(z, 2);
        }
    }
    const uint32_t ncount = bw.flush();
    if (bw.over || fse_build(d, d.wt, log, nsym) != OK) return 0;
    EncTab &t = st.wt;
    t.log = log;
    uint32_t cum = 0;
    PBSZ_ROLLED
    for (uint32_t w = 0; w < nsym; ++w) {
        t.p[w] = (uint8_t)d.norm[w];
        t.cum[w] = (uint8_t)cum;
        cum += (uint32_t)d.norm[w];
    }
    rank_states(t, d.wt);
    // two states in turn, the decoder's first one on the even weights; the last two weights are where the decoder ends:
    // their states take bits (the first state of a value takes the most, at least one), so its next read runs out
    bw.init(st.wdesc + 1 + ncount, 127 - ncount);
    const uint32_t e0 = t.state[t.cum[d.weights[nw - 1]]], e1 = t.state[t.cum[d.weights[nw - 2]]];
    uint32_t xa = ((nw - 1) & 1) ? e1 : e0, xb = ((nw - 1) & 1) ? e0 : e1;
    PBSZ_ROLLED
    for (uint32_t i = nw - 2; i > 0; --i) {
        if ((i - 1) & 1) fse_put(t, xb, d.weights[i - 1], bw);
        else fse_put(t, xa, d.weights[i - 1], bw);
    }
    bw.add(xb, log);
    bw.add(xa, log);
    const uint32_t len = bw.finish();
    if (bw.over) return 0;
    st.wdesc[0] = (uint8_t)(ncount + len);  // < 128
    return 1 + ncount + len;
}

// The literals section of lit[0, nlit) into blk[0, cap): its length, or kNone where it would not end before blk[cap].
template <class P>
PBSZ_HD uint32_t encode_literals(State &st, const uint8_t *lit, uint32_t nlit, uint8_t *blk, uint32_t cap) {
    uint32_t type = 0;  // raw
    if (nlit) {
        for (uint32_t i = (uint32_t)P::lane(); i < nlit; i += (uint32_t)P::lanes()) P::aadd(&st.hist[lit[i]], 1u);
        P::sync();
        if (P::lane() == 0) {
            uint32_t nsym = 0, maxsym = 0, maxcnt = 0;
            PBSZ_ROLLED
            for (uint32_t s = 0; s < 256; ++s) {
                const uint32_t c = st.hist[s];
                if (c) {
                    ++nsym;
                    maxsym = s;
                    if (c > maxcnt) maxcnt = c;
                }
            }
            st.nsym = nsym;
            st.maxsym = maxsym;
            st.maxcnt = maxcnt;
            st.sbits[0] = st.sbits[1] = st.sbits[2] = st.sbits[3] = 0;
        }
        P::sync();
        const uint32_t nsym = P::uni(st.nsym), maxsym = P::uni(st.maxsym);
        if (nsym == 1) {
            type = 1;
        } else {
            // byte values by ascending (count, value): each finds its own rank
            for (uint32_t s = (uint32_t)P::lane(); s < 256; s += (uint32_t)P::lanes()) {
                const uint32_t c = st.hist[s];
                st.len[s] = 0;
                if (!c) continue;
                uint32_t rank = 0;
                PBSZ_ROLLED
                for (uint32_t t = 0; t < 256; ++t) {
                    const uint32_t d = st.hist[t];
                    rank += (d && (d < c || (d == c && t < s))) ? 1u : 0u;
                }
                st.sorted[rank] = (uint8_t)s;
                st.key[rank] = c;
            }
            P::sync();
            if (P::lane() == 0) {
                huf_build(st, nsym);
                const uint32_t direct = maxsym <= 128 ? 1 + (maxsym + 1) / 2 : 0u;  // the byte 127 + maxsym, then four bits each
                const uint32_t fse = weights_fse(st, maxsym);
                st.wfse = fse && (!direct || fse < direct) ? 1u : 0u;
                st.desc = st.wfse ? fse : direct;  // 0: the weights cannot be described
            }
            P::sync();
            const uint32_t nstreams = nlit <= 1023 ? 1u : 4u, seg = (nlit + 3) / 4;
            for (uint32_t i = (uint32_t)P::lane(); i < nlit; i += (uint32_t)P::lanes()) {
                const uint32_t k = nstreams == 1 ? 0u : i / seg;
                P::aadd(&st.sbits[k], st.len[lit[i]]);
            }
            P::sync();
            const uint32_t desc = st.desc;  // (these five stay vector values: only what is branched on is made uniform)
            const uint32_t s0 = st.sbits[0] / 8 + 1, s1 = st.sbits[1] / 8 + 1, s2 = st.sbits[2] / 8 + 1,
                           s3 = st.sbits[3] / 8 + 1;  // with the end mark
            const uint32_t comp = P::uni(desc + (nstreams == 1 ? s0 : 6 + s0 + s1 + s2 + s3));
            if (comp >= nlit || !P::uni(st.desc)) {
                PBSZ_ECOV(E_HUF_REFUSED);
            } else {
                const uint32_t lh = nlit <= 1023 ? 3u : nlit <= 16383 ? 4u : 5u;
                if (lh + comp >= cap) return kNone;
                uint8_t *d = blk + lh + desc;
                if (P::lane() == 0) {
                    const uint32_t sf = nlit <= 1023 ? 0u : nlit <= 16383 ? 2u : 3u, bits = sf == 0 ? 10u : sf == 2 ? 14u : 18u;
                    const uint64_t v = 2u | sf << 2 | (uint64_t)nlit << 4 | (uint64_t)comp << (4 + bits);
                    for (uint32_t i = 0; i < lh; ++i) blk[i] = (uint8_t)(v >> (8 * i));
                    if (st.wfse) {
                        PBSZ_ROLLED
                        for (uint32_t i = 0; i < desc; ++i) blk[lh + i] = st.wdesc[i];
                    } else {
                        blk[lh] = (uint8_t)(127 + maxsym);
                        const uint32_t maxbits = st.maxbits;
                        PBSZ_ROLLED
                        for (uint32_t i = 0; i < maxsym; i += 2) {
                            const uint32_t la = st.len[i], lb = i + 1 < maxsym ? st.len[i + 1] : 0u;
                            const uint32_t wa = la ? maxbits + 1 - la : 0u, wb = lb ? maxbits + 1 - lb : 0u;
                            blk[lh + 1 + i / 2] = (uint8_t)(wa << 4 | wb);
                        }
                    }
                    if (nstreams == 4) {
                        d[0] = (uint8_t)s0;
                        d[1] = (uint8_t)(s0 >> 8);
                        d[2] = (uint8_t)s1;
                        d[3] = (uint8_t)(s1 >> 8);
                        d[4] = (uint8_t)s2;
                        d[5] = (uint8_t)(s2 >> 8);
                    }
                    PBSZ_ECOV(st.wfse ? E_WEIGHTS_FSE : E_WEIGHTS_DIRECT);
                    PBSZ_ECOV(nstreams == 1 ? E_HUF_1STREAM : E_HUF_4STREAM);
                }
                for (uint32_t k = (uint32_t)P::lane(); k < nstreams; k += (uint32_t)P::lanes()) {
                    const uint32_t from = nstreams == 1 ? 0u : k * seg, to = (nstreams == 1 || k == 3) ? nlit : from + seg;
                    const uint32_t at = nstreams == 1 ? 0u : 6 + (k > 0 ? s0 : 0u) + (k > 1 ? s1 : 0u) + (k > 2 ? s2 : 0u);
                    const uint32_t len = k == 0 ? s0 : k == 1 ? s1 : k == 2 ? s2 : s3;
                    BitWriter bw;
                    bw.init(d + at, len);
                    PBSZ_ROLLED
                    for (uint32_t i = to; i > from; --i) {
                        const uint32_t b = lit[i - 1];
                        bw.add(st.code[b], st.len[b]);
                    }
                    (void)bw.finish();
                }
                P::sync();
                return lh + comp;
            }
        }
    }
    // raw or RLE literals
    const uint32_t lh = nlit <= 31 ? 1u : nlit <= 4095 ? 2u : 3u;
    const uint32_t body = type == 1 ? 1u : nlit;
    if (lh + body >= cap) return kNone;
    if (P::lane() == 0) {
        const uint32_t v = lh == 1 ? (type | nlit << 3) : (type | (lh == 2 ? 1u : 3u) << 2 | nlit << 4);
        for (uint32_t i = 0; i < lh; ++i) blk[i] = (uint8_t)(v >> (8 * i));
        if (type == 1) blk[lh] = lit[0];
        PBSZ_ECOV(type == 1 ? E_LIT_RLE : E_LIT_RAW);
    }
    if (type == 0) copy_bytes<P>(blk + lh, lit, nlit);
    P::sync();
    return lh + body;
}

// The description of norm[0, nsym), which sums to 1 << log, as a forward bit stream (fse_read_norm, the other way round).
// weights_fse has the same loop in its own body and keeps it: taken out into this function, the block kernel of the other
// mode comes out of the compiler an instruction longer behind it, and that kernel is to stay the one it was.
PBSZ_HD void ncount_write(BitWriter &bw, const int16_t *norm, uint32_t nsym, uint32_t log) {
    bw.add(log - 5, 4);
    uint32_t remaining = 1u << log, s = 0;
    while (remaining > 0 && s < nsym) {
        const uint32_t R = remaining + 1, bits = highbit(R) + 1, lower = (1u << (bits - 1)) - 1, thr = (1u << bits) - 1 - R;
        const uint32_t p = (uint32_t)norm[s++], val = p + 1;
        if (val < thr) bw.add(val, bits - 1);
        else bw.add(val > lower ? val + thr : val, bits);
        remaining -= p;
        if (p == 0) {
            uint32_t z = 0;
            while (s < nsym && norm[s] == 0) {
                ++z;
                ++s;
            }
            while (z >= 3) {
                bw.add(3, 2);
                z -= 3;
            }
            bw.add(z, 2);
        }
    }
}

// log2(p) in 1/256, rounded down; 1 <= p <= 1 << 15. Eight squarings of the mantissa, one bit each: integers only, so both
// builds cost a table alike.
PBSZ_HD uint32_t log2_q8(uint32_t p) {
    const uint32_t hb = highbit(p);
    uint32_t x = p << (15 - hb), r = hb;  // x in [2^15, 2^16)
    PBSZ_ROLLED
    for (uint32_t i = 0; i < 8; ++i) {
        x = (x * x) >> 15;
        r <<= 1;
        if (x >> 16) {
            r |= 1;
            x >>= 1;
        }
    }
    return r;
}

// Lane 0, after the literals section (the hash table is dead: fse_build works in its bytes): the table of one symbol type
// for this block from st.shist[which], nseq >= 1 counts in all. Predefined_Mode unless one of the others is estimated to be
// shorter by more than the margin: kSeqMargin bits for the final state, whose width differs between the tables, and a
// 1/64 bit per sequence for the estimate itself, which is exact to 1/256 bit per code and assumes the states evenly used.
PBSZ_HD void choose_table(TState &st, uint32_t which, uint32_t nseq) {
    pbsz::State &d = st.u.dec;
    const EncTab &pre = which == 0 ? st.ll : which == 1 ? st.of : st.ml;
    const uint32_t npre = which == 0 ? 36u : which == 1 ? 29u : 53u, maxlog = which == 1 ? 8u : 9u;
    const uint32_t *cnt = st.shist[which];
    SeqTab &t = st.tab[which];
    uint32_t distinct = 0, nsym = 0, big = 0, cost0 = 0;
    PBSZ_ROLLED
    for (uint32_t s = 0; s < npre; ++s) {
        const uint32_t c = cnt[s];
        if (!c) continue;
        ++distinct;
        nsym = s + 1;
        if (c > cnt[big]) big = s;
        cost0 += c * ((pre.log << 8) - log2_q8(pre.p[s]));
    }
    const uint32_t margin = (kSeqMargin + nseq / 64) << 8;
    uint32_t mode = 0, log = 0, dlen = 0;
    if (distinct == 1) {
        if ((8u << 8) + margin < cost0) {
            mode = 1;
            dlen = 1;
            st.sdesc[which][0] = (uint8_t)big;
        }
    } else {
        // a state per 4 to 8 sequences, as far as the format lets the table grow; every code that occurs needs one
        log = nseq > 1 ? highbit(nseq - 1) : 0u;
        log = log < 7 ? 5u : log - 2 > maxlog ? maxlog : log - 2;
        while ((1u << log) < distinct) ++log;  // at most 6: 53 codes
        const uint32_t size = 1u << log;
        uint32_t sum = 0;
        PBSZ_ROLLED
        for (uint32_t s = 0; s < nsym; ++s) {
            const uint32_t c = cnt[s];
            uint32_t q = c ? (c * size + nseq / 2) / nseq : 0u;  // c <= kSeqCap, size <= 512: below 2^24
            if (c && !q) q = 1;
            d.norm[s] = (int16_t)q;
            sum += q;
        }
        while (sum > size) {  // rounding up overshot, by fewer than there are codes: off the largest, which stays above 1
            PBSZ_ROLLED
            for (uint32_t s = 0; s < nsym; ++s)
                if (d.norm[s] > d.norm[big]) big = s;
            d.norm[big]--;
            --sum;
        }
        d.norm[big] = (int16_t)(d.norm[big] + (int32_t)(size - sum));
        uint32_t cost2 = 0;
        PBSZ_ROLLED
        for (uint32_t s = 0; s < nsym; ++s)
            if (cnt[s]) cost2 += cnt[s] * ((log << 8) - log2_q8((uint32_t)d.norm[s]));
        BitWriter bw;
        bw.init(st.sdesc[which], kSeqDescMax);
        ncount_write(bw, d.norm, nsym, log);
        dlen = bw.flush();
        if (!bw.over && cost2 + (dlen << 11) + margin < cost0 && fse_build(d, d.ll, log, nsym) == OK) mode = 2;
    }
    st.smode[which] = mode;
    st.sdlen[which] = mode ? dlen : 0u;
    PBSZ_ECOV((which == 0 ? E_LL_PREDEF : which == 1 ? E_OF_PREDEF : E_ML_PREDEF) + (int)mode);
    if (mode == 2 && log == maxlog) PBSZ_ECOV(which == 0 ? E_LL_LOG_MAX : which == 1 ? E_OF_LOG_MAX : E_ML_LOG_MAX);
    if (mode == 0) {  // the predefined table in the wider form
        t.log = pre.log;
        PBSZ_ROLLED
        for (uint32_t u = 0; u < (1u << pre.log); ++u) t.state[u] = pre.state[u];
        PBSZ_ROLLED
        for (uint32_t s = 0; s < npre; ++s) {
            t.cum[s] = pre.cum[s];
            t.p[s] = pre.p[s];
        }
    } else if (mode == 1) {  // one state, no bits
        t.log = 0;
        t.state[0] = 0;
        t.cum[big] = 0;
        t.p[big] = 1;
    } else {
        t.log = log;
        uint32_t cum = 0;
        PBSZ_ROLLED
        for (uint32_t s = 0; s < nsym; ++s) {
            t.p[s] = (uint16_t)d.norm[s];
            t.cum[s] = (uint16_t)cum;
            cum += (uint32_t)d.norm[s];
        }
        rank_states(t, d.ll);
    }
}

// The block's tables (the mode with tables only): the three code streams counted by all lanes, then lane 0 chooses.
template <class P, class S>
PBSZ_HD void seq_tables(S &st, const uint64_t *seqs, uint32_t nseq) {
    for (uint32_t i = (uint32_t)P::lane(); i < 3 * 64; i += (uint32_t)P::lanes()) st.shist[i >> 6][i & 63] = 0;
    P::sync();
    for (uint32_t i = (uint32_t)P::lane(); i < nseq; i += (uint32_t)P::lanes()) {
        const uint64_t q = seqs[i];
        const uint32_t ll = (uint32_t)q & 0x3ffffu, ml = (uint32_t)(q >> 18) & 0x3ffffu, rc = (uint32_t)(q >> rep_shift<S>) & 3u;
        const uint32_t ov = rc ? rc : ((uint32_t)(q >> 36) & off_mask<S>) + 3;
        P::aadd(&st.shist[0][ll_code(ll)], 1u);
        P::aadd(&st.shist[1][highbit(ov)], 1u);
        P::aadd(&st.shist[2][ml_code(ml)], 1u);
    }
    P::sync();
    if (P::lane() == 0 && nseq) {
        choose_table(st, 0, nseq);
        choose_table(st, 1, nseq);
        choose_table(st, 2, nseq);
    }
    P::sync();
}

PBSZ_HD const EncTab &tab_ll(const State &st) { return st.ll; }
PBSZ_HD const EncTab &tab_of(const State &st) { return st.of; }
PBSZ_HD const EncTab &tab_ml(const State &st) { return st.ml; }
PBSZ_HD const SeqTab &tab_ll(const TState &st) { return st.tab[0]; }
PBSZ_HD const SeqTab &tab_of(const TState &st) { return st.tab[1]; }
PBSZ_HD const SeqTab &tab_ml(const TState &st) { return st.tab[2]; }

// Lane 0: the sequences section of seqs[0, nseq) into b[0, cap); its length, or kNone where it would not fit. With tables
// (S = TState, after seq_tables): the modes and descriptions the block chose, and the repeat codes of the words.
template <class S>
PBSZ_HD uint32_t encode_sequences(const S &st, const uint64_t *seqs, uint32_t nseq, uint8_t *b, uint32_t cap) {
    uint32_t p = 0;
    if (cap < 4) return kNone;
    if (nseq < 128) {
        b[p++] = (uint8_t)nseq;
        PBSZ_ECOV(nseq ? E_NSEQ_1 : E_NSEQ_0);
        if (!nseq) return p;
    } else {
        b[p++] = (uint8_t)((nseq >> 8) + 128);
        b[p++] = (uint8_t)nseq;
        PBSZ_ECOV(E_NSEQ_2);
    }
    if constexpr (S::kSeqTables) {
        if (cap - p < 1 + st.sdlen[0] + st.sdlen[1] + st.sdlen[2]) return kNone;
        b[p++] = (uint8_t)(st.smode[0] << 6 | st.smode[1] << 4 | st.smode[2] << 2);
        PBSZ_ROLLED
        for (uint32_t w = 0; w < 3; ++w) {
            PBSZ_ROLLED
            for (uint32_t i = 0; i < st.sdlen[w]; ++i) b[p++] = st.sdesc[w][i];
        }
    } else {
        b[p++] = 0;  // Predefined_Mode three times
    }
    const auto &t_ll = tab_ll(st);
    const auto &t_of = tab_of(st);
    const auto &t_ml = tab_ml(st);
    BitWriter bw;
    bw.init(b + p, cap - p);
    uint32_t x_ll = 0, x_of = 0, x_ml = 0;
    PBSZ_ROLLED
    for (uint32_t k = nseq; k-- > 0;) {
        const uint64_t q = seqs[k];
        const uint32_t ll = (uint32_t)q & 0x3ffffu, ml = (uint32_t)(q >> 18) & 0x3ffffu;
        uint32_t ov = (uint32_t)(q >> 36) + 3;
        if constexpr (S::kSeqTables) {
            const uint32_t rc = (uint32_t)(q >> rep_shift<S>) & 3u;
            ov = rc ? rc : ((uint32_t)(q >> 36) & off_mask<S>) + 3;
        }
        const uint32_t cl = ll_code(ll), cm = ml_code(ml), co = highbit(ov);
        if (k == nseq - 1) {  // the decoder ends in these states: any state of the symbol serves
            x_ll = t_ll.state[t_ll.cum[cl]];
            x_of = t_of.state[t_of.cum[co]];
            x_ml = t_ml.state[t_ml.cum[cm]];
        } else {
            fse_put(t_of, x_of, co, bw);
            fse_put(t_ml, x_ml, cm, bw);
            fse_put(t_ll, x_ll, cl, bw);
        }
        if (cl > 15) PBSZ_ECOV(E_LL_EXTRA);
        if (cm > 31) PBSZ_ECOV(E_ML_EXTRA);
        if (co >= 18) PBSZ_ECOV(E_W_OF_18);
        bw.add(ll - kLLBase[cl], kLLBits[cl]);
        bw.add(ml - kMLBase[cm], kMLBits[cm]);
        bw.add(ov - (1u << co), co);
        if (bw.over) return kNone;
    }
    bw.add(x_ml, t_ml.log);
    bw.add(x_of, t_of.log);
    bw.add(x_ll, t_ll.log);
    const uint32_t len = bw.finish();
    return bw.over ? kNone : p + len;
}

// Lane 0, the mode with repeat codes: the code (1..3, or 0 for the explicit offset + 3) of a match at `off` behind `ll`
// literals, and the block's history moved as the decoder moves its own (zstd_decode.h, decode_block). An entry is used only
// where this block has set it: what the blocks before left in the decoder is not known here.
PBSZ_HD uint32_t rep_code(uint32_t (&r)[3], uint32_t &known, uint32_t ll, uint32_t off) {
    const uint32_t k0 = known & 1u, k1 = known >> 1 & 1u, k2 = known >> 2 & 1u;
    const uint32_t r0 = r[0], r1 = r[1], r2 = r[2];
    uint32_t idx = 0;  // the decoder's: code + (ll == 0)
    if (ll && k0 && r0 == off) idx = 1;
    else if (k1 && r1 == off) idx = 2;
    else if (k2 && r2 == off) idx = 3;
    else if (!ll && k0 && r0 > 1 && r0 - 1 == off) idx = 4;
#ifdef PBSGPU_ZSTD_COVERAGE
    {
        uint32_t *g = g_dec_rep;
        const bool avail = (ll && g[0] == off) || g[1] == off || g[2] == off || (!ll && g[0] > 1 && g[0] - 1 == off);
        if (avail && !idx) PBSZ_ECOV(E_REP_UNKNOWN);
        if (idx) PBSZ_ECOV((ll ? E_REP_1 : E_REP0_1) + (int)idx - (ll ? 1 : 2));
        if (idx != 1) {  // (where idx names a known entry the decoder's holds the same value)
            if (idx != 2) g[2] = g[1];
            g[1] = g[0];
            g[0] = off;
        }
    }
#endif
    if (idx == 1) return 1;
    r[0] = off;
    r[1] = r0;
    r[2] = idx == 2 ? r2 : r1;
    known = 1u | k0 << 1 | (idx == 2 ? k2 : k1) << 2;
    return idx ? idx - (ll ? 0u : 1u) : 0u;
}

// One block src[0, bn), 1 <= bn <= kBlockMax: its type and, for a compressed block, the compressed form in blk[0, size).
// Returns type | size << 2 (size: payload_bytes), the same in every lane. init_tables has run on st. lit: kBlockMax bytes,
// seqs: kSeqCap words, blk: bn bytes; nothing else is stored to. S = TState: the mode with tables and repeat codes.
// S = WState or WTState, the long-range match finder: src[0, hn) is the block's history and src[hn, hn + bn) the block
// (positions are window-relative throughout), and wtab[0, 1 << kWindowHashLog) is the table, stored to as well.
template <class P, class S = State, class C = const uint8_t *>
PBSZ_HD uint32_t encode_block(S &st, const C src, uint32_t bn, uint8_t *blk, uint8_t *lit, uint64_t *seqs, uint32_t hn = 0,
                              uint32_t *wtab = nullptr) {
    constexpr uint32_t hlog = S::kWindow ? kWindowHashLog : kHashLog;
    uint32_t *const tab = S::kWindow ? wtab : st.u.hash;
    const uint32_t h0 = S::kWindow ? hn : 0u, end = h0 + bn;  // the block is src[h0, end)
    for (uint32_t i = (uint32_t)P::lane(); i < (1u << hlog); i += (uint32_t)P::lanes()) tab[i] = 0;
    for (uint32_t i = (uint32_t)P::lane(); i < 256; i += (uint32_t)P::lanes()) st.hist[i] = 0;
    if (P::lane() == 0) {
        st.flag = 0;
        st.cursor = h0;
        st.nlit = 0;
        st.nseq = 0;
        st.ll_run = 0;
        st.over = 0;
        st.size = 0;
        if constexpr (S::kSeqTables) {
            st.known = 0;  // nothing of the decoder's history is known at a block's start
            st.rep[0] = st.rep[1] = st.rep[2] = 0;
#ifdef PBSGPU_ZSTD_COVERAGE
            for (int i = 0; i < 3; ++i) g_dec_rep_block[i] = g_dec_rep[i];
#endif
        }
    }
    P::sync();
    const uint32_t first = P::uni(at(src, h0));
    for (uint32_t i = (uint32_t)P::lane(); i < bn; i += (uint32_t)P::lanes())
        if (at(src, h0 + i) != first) st.flag = 1;
    P::sync();
    if (!P::uni(st.flag)) {
        PBSZ_ECOV(E_BLOCK_RLE);
        return B_RLE | 1u << 2;
    }
    if constexpr (S::kWindow) {  // the history: every position whose four bytes lie in front of the block's end
        for (uint32_t l = (uint32_t)P::lane(); l < hn; l += (uint32_t)P::lanes())
            if (l + kMinMatch <= end) P::amax(&tab[hash4(rd32(src, l), hlog)], l + 1);
        P::sync();
    }
    for (uint32_t b0 = h0; b0 < end;) {
        // every position of the batch against the table as the batches before left it
        for (uint32_t l = (uint32_t)P::lane(); l < kLanes; l += (uint32_t)P::lanes()) {
            const uint32_t pos = b0 + l;
            uint32_t m = 0, off = 0, h = kNone;
            if (pos + kMinMatch <= end) {
                const uint32_t v = rd32(src, pos);
                h = hash4(v, hlog);
                const uint32_t c = tab[h];
                if (c && rd32(src, c, -1) == v) {
                    const uint32_t q = c - 1;  // q < pos
                    off = pos - q;
                    m = kMinMatch;
                    bool open = true;
                    while (open && pos + m + 4 <= end) {
                        const uint32_t x = rd32(src, q, m) ^ rd32(src, pos, m);
                        if (x) {
                            m += (uint32_t)__builtin_ctz(x) >> 3;
                            open = false;
                        } else {
                            m += 4;
                        }
                    }
                    while (open && pos + m < end && at(src, q, m) == at(src, pos, m)) ++m;
                    if constexpr (S::kWindow) {
                        if (q < h0) PBSZ_ECOV(E_W_CAND_HISTORY);
                        if (q < h0 && q + m > h0) PBSZ_ECOV(E_W_CROSS);
                    }
                }
            }
            st.mlen[l] = m;
            st.moff[l] = off;
            st.mh[l] = h;
        }
        P::sync();
        for (uint32_t l = (uint32_t)P::lane(); l < kLanes; l += (uint32_t)P::lanes())
            if (st.mh[l] != kNone) P::amax(&tab[st.mh[l]], b0 + l + 1);
        if (P::lane() == 0) {  // the matches in position order: the first at or after the cursor
            uint32_t cursor = st.cursor, nlit = st.nlit, nseq = st.nseq, run = st.ll_run;
            PBSZ_ROLLED
            for (uint32_t l = 0; l < kLanes; ++l) {
                const uint32_t pos = b0 + l;
                uint32_t at_lit = kNone;
                if (pos < end && pos >= cursor) {
                    const uint32_t m = st.mlen[l];
                    if (m >= kMinMatch && nseq < kSeqCap) {
                        const uint32_t off = st.moff[l];
                        if (off < m) PBSZ_ECOV(E_MATCH_OVERLAP);
                        if (off == 1) PBSZ_ECOV(E_MATCH_OFFSET_1);
                        uint64_t q = (uint64_t)run | (uint64_t)m << 18 | (uint64_t)off << 36;
                        if constexpr (S::kSeqTables) q |= (uint64_t)rep_code(st.rep, st.known, run, off) << rep_shift<S>;
                        seqs[nseq++] = q;
                        run = 0;
                        cursor = pos + m;
                    } else {
                        if (m >= kMinMatch) PBSZ_ECOV(E_SEQ_CAP);
                        at_lit = nlit++;
                        ++run;
                    }
                }
                st.lidx[l] = at_lit;
            }
            st.cursor = cursor;
            st.nlit = nlit;
            st.nseq = nseq;
            st.ll_run = run;
            st.next_b0 = cursor > b0 + kLanes ? cursor : b0 + kLanes;
        }
        P::sync();
        for (uint32_t l = (uint32_t)P::lane(); l < kLanes; l += (uint32_t)P::lanes())
            if (st.lidx[l] != kNone) lit[st.lidx[l]] = at(src, b0 + l);
        b0 = P::uni(st.next_b0);
    }
    P::sync();
    const uint32_t nlit = P::uni(st.nlit), nseq = P::uni(st.nseq);
    uint32_t type = B_RAW, size = bn;
    const uint32_t lsize = encode_literals<P>(st, lit, nlit, blk, bn);
    if (lsize != kNone) {
        if constexpr (S::kSeqTables) seq_tables<P, S>(st, seqs, nseq);
        if (P::lane() == 0) st.size = encode_sequences(st, seqs, nseq, blk + lsize, bn - lsize);
        P::sync();
        const uint32_t ssize = P::uni(st.size);
        if (ssize != kNone && lsize + ssize < bn) {
            type = B_COMPRESSED;
            size = lsize + ssize;
        }
    }
    PBSZ_ECOV(type == B_RAW ? E_BLOCK_RAW : E_BLOCK_COMPRESSED);
#ifdef PBSGPU_ZSTD_COVERAGE
    if constexpr (S::kSeqTables)
        if (type == B_RAW)  // its sequences never reach the decoder
            for (int i = 0; i < 3; ++i) g_dec_rep[i] = g_dec_rep_block[i];
#endif
    return type | size << 2;
}

// The frame of src[0, n), n < 4 GiB, into dst[0, room): BAD_SIZE where it needs more, and dst's contents are then
// unspecified. *flen = the frame's length (with OK). Scratch as for encode_block. Never stores outside dst[0, room) and
// the scratch. The long-range match finder (S = WState or WTState) also takes the window's log and its table, and the
// content may lie in two parts (C = Src2). sum: where the caller has put XXH64(content, 0) (xxh64.h; the kernels take it
// from k_xxh64_ranges), and the frame then carries the content checksum: the flag in its header, the low word behind its
// last block. nullptr: the frame without, byte for byte what it always was.
template <class P, class S = State, class C = const uint8_t *>
PBSZ_HD int encode_frame(S &st, const C src, uint32_t n, uint8_t *dst, uint64_t room, uint8_t *blk, uint8_t *lit,
                         uint64_t *seqs, uint64_t *flen, uint32_t window_log = 0, uint32_t *wtab = nullptr,
                         const uint64_t *sum = nullptr) {
    *flen = 0;
#ifdef PBSGPU_ZSTD_COVERAGE
    g_dec_rep[0] = 1, g_dec_rep[1] = 4, g_dec_rep[2] = 8;  // a frame's decoder starts here
#endif
    init_tables<P>(st);
    const uint32_t hb = header_bytes(n);
    if (room < (uint64_t)hb + 3) return BAD_SIZE;
    if (P::lane() == 0) frame_header(n, dst, sum != nullptr);
    uint64_t pos = hb;
    auto close = [&]() -> int {  // the checksum, if any, and the length
        PBSZ_COV2(sum ? K_ENC_SUM : K_ENC_NO_SUM);
        if (sum) {
            if (room - pos < 4) {
                PBSZ_COV2(K_ENC_SUM_NO_ROOM);
                return BAD_SIZE;
            }
            if (P::lane() == 0)
                for (uint32_t i = 0; i < 4; ++i) dst[pos + i] = (uint8_t)(*sum >> (8 * i));
            pos += 4;
            P::sync();
        }
        *flen = pos;
        return OK;
    };
    if (n == 0) {
        if (P::lane() == 0) block_header(dst + pos, 1, B_RAW, 0);
        PBSZ_ECOV(E_EMPTY_LAST_BLOCK);
        P::sync();
        pos += 3;
        return close();
    }
    for (uint32_t at = 0; at < n; at += kBlockMax) {
        const uint32_t bn = n - at < kBlockMax ? n - at : kBlockMax;
        uint32_t r;
        if constexpr (S::kWindow) {  // the history: what of the window lies in the chunk
            const uint32_t hn = at < (1u << window_log) ? at : 1u << window_log;
            if (hn < at) PBSZ_ECOV(E_W_BEYOND);
            else if (at) PBSZ_ECOV(E_W_CHUNK_START);
            r = encode_block<P, S>(st, from(src, at - hn), bn, blk, lit, seqs, hn, wtab);
        } else {
            r = encode_block<P, S>(st, from(src, at), bn, blk, lit, seqs);
        }
        const uint32_t type = r & 3u, size = r >> 2;
        if (room - pos < (uint64_t)3 + size) return BAD_SIZE;
        if (P::lane() == 0) block_header(dst + pos, at + bn == n ? 1u : 0u, type, type == B_COMPRESSED ? size : bn);
        pos += 3;
        if (type == B_RLE) {
            if (P::lane() == 0) dst[pos] = enc::at(src, at);
        } else if (type == B_RAW) {
            for (uint32_t i = (uint32_t)P::lane(); i < size; i += (uint32_t)P::lanes()) dst[pos + i] = enc::at(src, at + i);
        } else {
            copy_bytes<P>(dst + pos, blk, size);
        }
        pos += size;
        P::sync();  // blk, lit and seqs go to the next block
    }
    return close();
}

}  // namespace enc
}  // namespace pbsz
