// AES-256-GCM with an empty AAD and a 16-byte tag, the cipher of PBS's encrypted data blobs: ONE implementation, compiled
// twice, in the manner of zstd_decode.h and xxh64.h. Under hipcc every function is __host__ __device__ and aes_gcm.hip
// runs it; without hipcc it is plain inline C++, and that build is what tests/native/test_aes_gcm.cpp runs under
// AddressSanitizer. No HIP and no libc beyond the fixed-width integers.
//
// A 16-byte block is four big-endian words (Blk), w[0] first: the AES state's columns, and a GF(2^128) element in GCM's
// bit order, in which the coefficient of x^0 is the top bit of w[0] and "times x" is a shift to the RIGHT.
//
// AES: the forward cipher only, from ONE table of 256 words (te0[b] = 2s, s, s, 3s with s = sbox[b]); the other three
// tables of the usual form are its rotations, and the last round takes the plain S-box from its second byte. gfx950 has
// no AES instruction: the kernel keeps te0 in LDS (1 KiB). THE TABLE IS INDEXED BY SECRET-DEPENDENT BYTES: a timing
// channel that is not addressed here.
//
// GHASH is a chain over the message, Y = (Y ^ C_i) * H. It is cut twice:
//   * a message into PIECES of kPiece bytes counted from its start. A piece of m blocks has the partial
//     P = sum C_j * H^(m-1-j); the message's hash is (sum over pieces P * H^(blocks behind the piece + 1) ^ LEN) * H.
//   * a piece over kStride LANES that take interleaved blocks (lane t: t, t + kStride, ...) and run Horner with the ONE
//     multiplier H^kStride, through a table (mul_tab: 256 entries b * H^kStride and the 256 reductions of the byte that a
//     shift by eight pushes out; 5 KiB in LDS). A lane's sum is then moved to the piece's end with H^(m-1-its last block),
//     a power below kStride that the key holds, by the plain shift-and-xor multiply (mul), once per lane and piece.
// piece_lane is that lane, CTR included; the kernel and the CPU program call the same function, so the CPU program checks
// "pieces + fold = the serial chain" with the code the kernels run.
//
// The pre-counter block J0 is IV || 0^31 1 for a 12-byte IV and GHASH(IV padded || 0^64 || [bits of IV]_64) for every
// other length (PBS uses 16 bytes), so its low word is arbitrary and inc32 may wrap inside a message: ctr_add wraps the
// low word alone.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define PBSA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PBSA_HD inline
#endif

#if defined(__clang__)
#define PBSA_ROLLED _Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
#elif defined(__GNUC__)
#define PBSA_ROLLED _Pragma("GCC unroll 1")
#else
#define PBSA_ROLLED
#endif

#ifdef PBSGPU_AES_COVERAGE  // CPU test build only: one bit per branch (names: tests/test_aes_gcm_native.py)
namespace pbsa {
inline uint64_t g_cov = 0;
}
#define PBSA_COV(bit) (::pbsa::g_cov |= 1ull << (bit))
#else
#define PBSA_COV(bit) ((void)0)
#endif

namespace pbsa {

enum : int { OK = 0, BAD_TAG = 1 };

enum : int {  // coverage bits
    A_IV_12, A_IV_BLOCKS, A_IV_PART, A_BLOCK_FULL, A_BLOCK_PART, A_LANE_IDLE, A_LANE_ONE, A_LANE_MANY, A_LANE_AT_END,
    A_LANE_MOVED, A_CTR_WRAP, A_POW_BIT_SET, A_POW_BIT_CLEAR, A_EMPTY, A_TAG_GOOD, A_TAG_BAD, A_ENCRYPT, A_DECRYPT,
    A_NBITS
};

constexpr uint32_t kPiece = 64u << 10;             // bytes of a message that one workgroup carries
constexpr uint32_t kPieceBlocks = kPiece / 16;
constexpr uint32_t kStride = 256;                  // lanes of a piece: the workgroup's size
constexpr uint32_t kPow2 = 32;                     // H^(2^k), k < kPow2: a message has fewer than 2^28 blocks

struct alignas(16) Blk {  // (aligned: a table entry is one 16-byte load)
    uint32_t w[4];
};

PBSA_HD Blk bxor(Blk a, Blk b) { return Blk{{a.w[0] ^ b.w[0], a.w[1] ^ b.w[1], a.w[2] ^ b.w[2], a.w[3] ^ b.w[3]}}; }
PBSA_HD uint32_t bswap(uint32_t v) { return __builtin_bswap32(v); }

// sixteen bytes at any alignment (gfx950 loads unaligned words from global memory)
PBSA_HD Blk load_be(const uint8_t *p) {
    Blk b;
    __builtin_memcpy(&b, p, 16);
    for (int i = 0; i < 4; ++i) b.w[i] = bswap(b.w[i]);
    return b;
}
PBSA_HD void store_be(uint8_t *p, Blk b) {
    for (int i = 0; i < 4; ++i) b.w[i] = bswap(b.w[i]);
    __builtin_memcpy(p, &b, 16);
}
// the first n < 16 bytes, the rest zero; and back. Byte by byte: nothing outside p[0, n) is touched
PBSA_HD Blk load_be_part(const uint8_t *p, uint32_t n) {
    Blk b{{0, 0, 0, 0}};
    PBSA_ROLLED
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t v = (uint32_t)p[i] << (24 - 8 * (i & 3));
        b.w[0] |= (i >> 2) == 0 ? v : 0;  // (selects, not an indexed store: the block stays in registers)
        b.w[1] |= (i >> 2) == 1 ? v : 0;
        b.w[2] |= (i >> 2) == 2 ? v : 0;
        b.w[3] |= (i >> 2) == 3 ? v : 0;
    }
    return b;
}
PBSA_HD uint32_t word_of(const Blk &b, uint32_t i) {  // b.w[i] by selects
    return i == 0 ? b.w[0] : i == 1 ? b.w[1] : i == 2 ? b.w[2] : b.w[3];
}
PBSA_HD uint32_t byte_of(const Blk &b, uint32_t i) { return word_of(b, i >> 2) >> (24 - 8 * (i & 3)) & 0xffu; }
PBSA_HD void store_be_part(uint8_t *p, const Blk &b, uint32_t n) {
    PBSA_ROLLED
    for (uint32_t i = 0; i < n; ++i) p[i] = (uint8_t)byte_of(b, i);
}
PBSA_HD Blk keep_bytes(Blk b, uint32_t n) {  // the first n <= 16 bytes, the rest zero
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t have = n > 4 * k ? n - 4 * k : 0;
        b.w[k] &= have >= 4 ? 0xffffffffu : have == 0 ? 0u : ~(0xffffffffu >> (8 * have));
    }
    return b;
}

// ---- AES-256, forward ----

constexpr int kRounds = 14;
constexpr int kRkWords = 4 * (kRounds + 1);

PBSA_HD uint32_t ror(uint32_t v, int r) { return v >> r | v << (32 - r); }
PBSA_HD uint32_t sub(const uint32_t *te0, uint32_t b) { return te0[b] >> 8 & 0xffu; }  // the S-box

// te0 from the field arithmetic (no table in the source): sbox = affine(inverse), p walks the generator 3, q its inverse
inline void make_te0(uint32_t te0[256]) {
    uint8_t sbox[256];
    uint8_t p = 1, q = 1;
    do {
        p = (uint8_t)(p ^ (p << 1) ^ ((p & 0x80) ? 0x1B : 0));
        q ^= (uint8_t)(q << 1);
        q ^= (uint8_t)(q << 2);
        q ^= (uint8_t)(q << 4);
        if (q & 0x80) q ^= 0x09;
        const uint8_t r1 = (uint8_t)(q << 1 | q >> 7), r2 = (uint8_t)(q << 2 | q >> 6), r3 = (uint8_t)(q << 3 | q >> 5),
                      r4 = (uint8_t)(q << 4 | q >> 4);
        sbox[p] = (uint8_t)(q ^ r1 ^ r2 ^ r3 ^ r4 ^ 0x63);
    } while (p != 1);
    sbox[0] = 0x63;
    for (int i = 0; i < 256; ++i) {
        const uint32_t s = sbox[i], s2 = (s << 1 ^ ((s & 0x80) ? 0x11B : 0)) & 0xffu;
        te0[i] = s2 << 24 | s << 16 | s << 8 | (s2 ^ s);
    }
}

inline void expand_key(const uint8_t key[32], const uint32_t *te0, uint32_t rk[kRkWords]) {
    for (int i = 0; i < 8; ++i)
        rk[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 | (uint32_t)key[4 * i + 2] << 8 | key[4 * i + 3];
    uint32_t rcon = 1;
    for (int i = 8; i < kRkWords; ++i) {
        uint32_t t = rk[i - 1];
        if (i % 8 == 0) {
            t = t << 8 | t >> 24;
            t = sub(te0, t >> 24) << 24 | sub(te0, t >> 16 & 0xff) << 16 | sub(te0, t >> 8 & 0xff) << 8 | sub(te0, t & 0xff);
            t ^= rcon << 24;
            rcon = (rcon << 1 ^ ((rcon & 0x80) ? 0x11B : 0)) & 0xffu;
        } else if (i % 8 == 4) {
            t = sub(te0, t >> 24) << 24 | sub(te0, t >> 16 & 0xff) << 16 | sub(te0, t >> 8 & 0xff) << 8 | sub(te0, t & 0xff);
        }
        rk[i] = rk[i - 8] ^ t;
    }
}

PBSA_HD Blk encrypt_block(const uint32_t *rk, const uint32_t *te0, Blk in) {
    uint32_t s0 = in.w[0] ^ rk[0], s1 = in.w[1] ^ rk[1], s2 = in.w[2] ^ rk[2], s3 = in.w[3] ^ rk[3];
    PBSA_ROLLED
    for (int r = 1; r < kRounds; ++r) {
        const uint32_t *k = rk + 4 * r;
        const uint32_t t0 = te0[s0 >> 24] ^ ror(te0[s1 >> 16 & 0xff], 8) ^ ror(te0[s2 >> 8 & 0xff], 16) ^ ror(te0[s3 & 0xff], 24) ^ k[0];
        const uint32_t t1 = te0[s1 >> 24] ^ ror(te0[s2 >> 16 & 0xff], 8) ^ ror(te0[s3 >> 8 & 0xff], 16) ^ ror(te0[s0 & 0xff], 24) ^ k[1];
        const uint32_t t2 = te0[s2 >> 24] ^ ror(te0[s3 >> 16 & 0xff], 8) ^ ror(te0[s0 >> 8 & 0xff], 16) ^ ror(te0[s1 & 0xff], 24) ^ k[2];
        const uint32_t t3 = te0[s3 >> 24] ^ ror(te0[s0 >> 16 & 0xff], 8) ^ ror(te0[s1 >> 8 & 0xff], 16) ^ ror(te0[s2 & 0xff], 24) ^ k[3];
        s0 = t0, s1 = t1, s2 = t2, s3 = t3;
    }
    const uint32_t *k = rk + 4 * kRounds;
    Blk o;
    o.w[0] = (sub(te0, s0 >> 24) << 24 | sub(te0, s1 >> 16 & 0xff) << 16 | sub(te0, s2 >> 8 & 0xff) << 8 | sub(te0, s3 & 0xff)) ^ k[0];
    o.w[1] = (sub(te0, s1 >> 24) << 24 | sub(te0, s2 >> 16 & 0xff) << 16 | sub(te0, s3 >> 8 & 0xff) << 8 | sub(te0, s0 & 0xff)) ^ k[1];
    o.w[2] = (sub(te0, s2 >> 24) << 24 | sub(te0, s3 >> 16 & 0xff) << 16 | sub(te0, s0 >> 8 & 0xff) << 8 | sub(te0, s1 & 0xff)) ^ k[2];
    o.w[3] = (sub(te0, s3 >> 24) << 24 | sub(te0, s0 >> 16 & 0xff) << 16 | sub(te0, s1 >> 8 & 0xff) << 8 | sub(te0, s2 & 0xff)) ^ k[3];
    return o;
}

// ---- GF(2^128), GCM's bit order ----

constexpr uint32_t kPolyTop = 0xE1000000u;  // x^128 = x^7 + x^2 + x + 1, as the top byte of w[0]

PBSA_HD Blk gf_one() { return Blk{{0x80000000u, 0, 0, 0}}; }
PBSA_HD Blk mulx(Blk v) {
    const uint32_t out = 0u - (v.w[3] & 1u);
    v.w[3] = v.w[3] >> 1 | v.w[2] << 31;
    v.w[2] = v.w[2] >> 1 | v.w[1] << 31;
    v.w[1] = v.w[1] >> 1 | v.w[0] << 31;
    v.w[0] = v.w[0] >> 1 ^ (out & kPolyTop);
    return v;
}
// x * y by 128 shifts and masked xors: no table, for the few multiplies off the block chain
PBSA_HD Blk mul(Blk x, Blk y) {
    Blk z{{0, 0, 0, 0}};
    for (int k = 0; k < 4; ++k) {
        uint32_t bits = x.w[k];
        PBSA_ROLLED
        for (int i = 0; i < 32; ++i) {
            const uint32_t m = 0u - (bits >> 31);
            z.w[0] ^= y.w[0] & m, z.w[1] ^= y.w[1] & m, z.w[2] ^= y.w[2] & m, z.w[3] ^= y.w[3] & m;
            bits <<= 1;
            y = mulx(y);
        }
    }
    return z;
}

// the table form for ONE multiplier M: tab[b] = (b as the element's first byte) * M, red[b] = what byte b, pushed out at
// the low end by a shift of eight, adds at the top (the top 16 bits of w[0])
inline void make_red(uint32_t red[256]) {
    for (uint32_t b = 0; b < 256; ++b) {
        Blk e{{0, 0, 0, b}};
        for (int i = 0; i < 8; ++i) e = mulx(e);
        red[b] = e.w[0];
    }
}
inline void make_tab(Blk m, Blk tab[256]) {
    tab[0] = Blk{{0, 0, 0, 0}};
    Blk v = m;
    for (uint32_t b = 0x80; b; b >>= 1, v = mulx(v)) tab[b] = v;  // 0x80 is x^0
    for (uint32_t b = 1; b < 256; ++b)
        if (b & (b - 1)) tab[b] = bxor(tab[b & (b - 1)], tab[b & (0u - b)]);
}
PBSA_HD Blk mul_tab(Blk x, const Blk *tab, const uint32_t *red) {
    Blk z = tab[x.w[3] & 0xffu];
    PBSA_ROLLED
    for (int i = 14; i >= 0; --i) {
        const uint32_t out = z.w[3] & 0xffu;
        z.w[3] = z.w[3] >> 8 | z.w[2] << 24;
        z.w[2] = z.w[2] >> 8 | z.w[1] << 24;
        z.w[1] = z.w[1] >> 8 | z.w[0] << 24;
        z.w[0] = z.w[0] >> 8 ^ red[out];
        z = bxor(z, tab[byte_of(x, (uint32_t)i)]);
    }
    return z;
}

// h^n by squaring: the host's way to any power (the key's tables), checked against repeated multiplication
PBSA_HD Blk gf_pow(Blk h, uint64_t n) {
    Blk r = gf_one();
    PBSA_ROLLED
    for (; n; n >>= 1, h = mul(h, h))
        if (n & 1) r = mul(r, h);
    return r;
}
// x * H^n from pow2[k] = H^(2^k): one multiply per set bit of n
PBSA_HD Blk mul_pow(Blk x, uint64_t n, const Blk *pow2) {
    PBSA_ROLLED
    for (uint32_t k = 0; n; n >>= 1, ++k) {
        if (n & 1) {
            PBSA_COV(A_POW_BIT_SET);
            x = mul(x, pow2[k]);
        } else {
            PBSA_COV(A_POW_BIT_CLEAR);
        }
    }
    return x;
}

// ---- what a key holds (built on the host, read by the kernels from device memory) ----

struct KeyTables {
    uint32_t te0[256];
    uint32_t red[256];
    Blk stride[256];     // the table of H^kStride
    Blk low[kStride];    // H^0 .. H^(kStride-1)
    Blk pow2[kPow2];     // H^(2^k)
    uint32_t rk[kRkWords];
    Blk h;               // E_K(0)
};

inline void make_key(const uint8_t key[32], KeyTables &kt) {
    make_te0(kt.te0);
    make_red(kt.red);
    expand_key(key, kt.te0, kt.rk);
    kt.h = encrypt_block(kt.rk, kt.te0, Blk{{0, 0, 0, 0}});
    kt.low[0] = gf_one();
    for (uint32_t i = 1; i < kStride; ++i) kt.low[i] = mul(kt.low[i - 1], kt.h);
    make_tab(mul(kt.low[kStride - 1], kt.h), kt.stride);
    kt.pow2[0] = kt.h;
    for (uint32_t k = 1; k < kPow2; ++k) kt.pow2[k] = mul(kt.pow2[k - 1], kt.pow2[k - 1]);
}

// ---- the counter ----

PBSA_HD Blk ghash_step(Blk y, Blk c, Blk h) { return mul(bxor(y, c), h); }  // the serial chain, one block

PBSA_HD Blk j0_of(Blk h, const uint8_t *iv, uint32_t n) {
    if (n == 12) {
        PBSA_COV(A_IV_12);
        Blk b = load_be_part(iv, 12);
        b.w[3] = 1;
        return b;
    }
    Blk y{{0, 0, 0, 0}};
    uint32_t i = 0;
    for (; i + 16 <= n; i += 16) {
        PBSA_COV(A_IV_BLOCKS);
        y = ghash_step(y, load_be_part(iv + i, 16), h);  // (bytes: the IV table has no alignment)
    }
    if (i < n) {
        PBSA_COV(A_IV_PART);
        y = ghash_step(y, load_be_part(iv + i, n - i), h);
    }
    return ghash_step(y, Blk{{0, 0, n >> 29, n << 3}}, h);
}
PBSA_HD Blk ctr_add(Blk j0, uint32_t n) {  // inc32, n times: the low word wraps alone
    if (j0.w[3] + n < j0.w[3]) PBSA_COV(A_CTR_WRAP);
    j0.w[3] += n;
    return j0;
}

// ---- a piece ----

// Lane `lane` of kStride on piece `piece` of a message: in/out point at the PIECE's first byte, plen (1..kPiece) is its
// length. CTR over the lane's blocks (in ^ keystream -> out, exactly plen bytes in all) and the lane's share of the
// piece's partial hash of the CIPHERTEXT, moved to the piece's end. The xor over all lanes is the piece's partial.
// store = false writes nothing: the tag of a ciphertext can be checked without room for its plaintext.
PBSA_HD Blk piece_lane(const uint32_t *rk, const uint32_t *te0, const Blk *stride, const uint32_t *red, const Blk *low, Blk j0,
                       uint32_t piece, const uint8_t *in, uint8_t *out, uint32_t plen, bool encrypt, uint32_t lane,
                       bool store = true) {
    const uint32_t m = (plen + 15) / 16;
    Blk y{{0, 0, 0, 0}};
    if (lane >= m) {
        PBSA_COV(A_LANE_IDLE);
        return y;
    }
    uint32_t j = lane;
    PBSA_ROLLED
    for (; j < m; j += kStride) {
        const Blk ks = encrypt_block(rk, te0, ctr_add(j0, 1u + piece * kPieceBlocks + j));
        const uint32_t n = plen - 16 * j < 16 ? plen - 16 * j : 16;
        Blk c;
        if (n == 16) {
            PBSA_COV(A_BLOCK_FULL);
            c = load_be(in + 16 * (uint64_t)j);
            const Blk o = bxor(c, ks);
            if (store) store_be(out + 16 * (uint64_t)j, o);
            if (encrypt) c = o;
        } else {
            PBSA_COV(A_BLOCK_PART);
            c = load_be_part(in + 16 * (uint64_t)j, n);
            const Blk o = keep_bytes(bxor(c, ks), n);
            if (store) store_be_part(out + 16 * (uint64_t)j, o, n);
            if (encrypt) c = o;
        }
        if (j == lane) {
            PBSA_COV(A_LANE_ONE);
            y = c;
        } else {
            PBSA_COV(A_LANE_MANY);
            y = bxor(mul_tab(y, stride, red), c);
        }
    }
    const uint32_t behind = m - 1 - (j - kStride);  // blocks of the piece behind the lane's last one: below kStride
    if (behind == 0) {
        PBSA_COV(A_LANE_AT_END);
        return y;
    }
    PBSA_COV(A_LANE_MOVED);
    return mul(y, low[behind]);
}

PBSA_HD uint32_t pieces_of(uint32_t len) { return (uint32_t)(((uint64_t)len + kPiece - 1) / kPiece); }
PBSA_HD uint32_t piece_len(uint32_t len, uint32_t piece) {
    const uint32_t left = len - piece * kPiece;
    return left < kPiece ? left : kPiece;
}
// piece `piece`'s term of a message of len bytes: its partial times H^(blocks behind the piece + 1)
PBSA_HD Blk fold_piece(Blk partial, uint32_t len, uint32_t piece, const Blk *pow2) {
    const uint64_t blocks = ((uint64_t)len + 15) / 16, upto = (uint64_t)(piece + 1) * kPieceBlocks;
    return mul_pow(partial, (upto < blocks ? blocks - upto : 0) + 1, pow2);
}
// the tag from the xor of all terms: (terms ^ LEN) * H ^ E_K(J0)
PBSA_HD Blk tag_of(Blk terms, uint32_t len, Blk h, Blk ekj0) {
    if (len == 0) PBSA_COV(A_EMPTY);
    return bxor(mul(bxor(terms, Blk{{0, 0, len >> 29, len << 3}}), h), ekj0);
}
// BAD_TAG unless all sixteen bytes agree; every byte is looked at
PBSA_HD int tag_verdict(Blk a, Blk b) {
    const uint32_t d = (a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3]);
    if (d) {
        PBSA_COV(A_TAG_BAD);
        return BAD_TAG;
    }
    PBSA_COV(A_TAG_GOOD);
    return OK;
}

// One message on one thread, by pieces and fold: what the kernels compute, in their order. in/out: len bytes. Encrypting
// writes tag; decrypting compares it and, on a bad tag, zeroes out[0, len). Returns OK or BAD_TAG.
inline int crypt_by_pieces(const KeyTables &kt, const uint8_t *iv, uint32_t iv_len, const uint8_t *in, uint8_t *out,
                           uint32_t len, bool encrypt, uint8_t tag[16]) {
    PBSA_COV(encrypt ? A_ENCRYPT : A_DECRYPT);
    const Blk j0 = j0_of(kt.h, iv, iv_len), ekj0 = encrypt_block(kt.rk, kt.te0, j0);
    Blk terms{{0, 0, 0, 0}};
    for (uint32_t p = 0; p < pieces_of(len); ++p) {
        Blk part{{0, 0, 0, 0}};
        for (uint32_t lane = 0; lane < kStride; ++lane)
            part = bxor(part, piece_lane(kt.rk, kt.te0, kt.stride, kt.red, kt.low, j0, p, in + (uint64_t)p * kPiece,
                                         out + (uint64_t)p * kPiece, piece_len(len, p), encrypt, lane));
        terms = bxor(terms, fold_piece(part, len, p, kt.pow2));
    }
    const Blk t = tag_of(terms, len, kt.h, ekj0);
    if (encrypt) {
        store_be(tag, t);
        return OK;
    }
    const int v = tag_verdict(t, load_be_part(tag, 16));
    if (v != OK)
        for (uint32_t i = 0; i < len; ++i) out[i] = 0;
    return v;
}

// The same message by the definition: one CTR stream, one GHASH chain with the plain multiply, no table and no piece.
// The CPU program's yardstick for crypt_by_pieces. Writes the tag it computes to tag_out in both directions.
inline void crypt_serial(const KeyTables &kt, const uint8_t *iv, uint32_t iv_len, const uint8_t *in, uint8_t *out, uint32_t len,
                         bool encrypt, uint8_t tag_out[16]) {
    const Blk j0 = j0_of(kt.h, iv, iv_len);
    Blk y{{0, 0, 0, 0}};
    for (uint32_t off = 0, j = 0; off < len; off += 16, ++j) {
        const uint32_t n = len - off < 16 ? len - off : 16;
        const Blk ks = encrypt_block(kt.rk, kt.te0, ctr_add(j0, 1u + j));
        const Blk c = load_be_part(in + off, n), o = keep_bytes(bxor(c, ks), n);
        store_be_part(out + off, o, n);
        y = ghash_step(y, encrypt ? o : c, kt.h);
    }
    y = ghash_step(y, Blk{{0, 0, len >> 29, len << 3}}, kt.h);
    store_be(tag_out, bxor(y, encrypt_block(kt.rk, kt.te0, j0)));
}

}  // namespace pbsa
