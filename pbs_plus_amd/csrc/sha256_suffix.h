// The tail of a KEYED chunk digest, SHA-256(content || key): what every byte of a block that is not 64 full data bytes is.
// An encrypted backup names a chunk by SHA-256(content || id_key), 32 secret bytes appended behind the content (INTEGRATION.md
// §6), so the padding-only block(s) of the plain digest become
//     last data bytes | 32 key bytes | 0x80 | zeros | big-endian bit length of len + 32.
// One function, registers only, no memory access: the kernels (kernels.hip, sha256_tail_words_keyed) assemble the block's data
// words with their own clamped global loads and call it; tests/native/test_sha256_suffix.cpp calls it on the CPU under the
// sanitizers. Words are RAW little-endian throughout (byte k of the block in bits 8 * (k & 3) of word k / 4), as the
// kernels hold a block before the byte swap.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PBSS_HD __host__ __device__ __forceinline__
#else
#define PBSS_HD inline
#endif

namespace pbss {

constexpr uint32_t kSuffixBytes = 32;  // the key's length: a compile-time constant of the keyed kernels
constexpr uint32_t kSuffixWords = kSuffixBytes / 4;

// blocks of a chunk of `len` bytes whose digest covers `suffix` more bytes: data + suffix, the marker, the 8-byte length
PBSS_HD uint64_t sha256_blocks(uint64_t len, uint32_t suffix) { return (len + suffix + 8) / 64 + 1; }

PBSS_HD uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

// d:     the block's data words, bytes off .. off + 63 of the chunk; only the first `valid` bytes are looked at
// valid: data bytes in this block, 0 .. 63 (a block of 64 data bytes never comes here)
// len:   the chunk's length, off: the block's offset in the chunk (a multiple of 64), off + 64 > len
// key:   the eight key words, raw little-endian like the data
// last:  this is the chunk's last block (block sha256_blocks(len, 32) - 1): it ends with the bit length
// out:   the block's sixteen words
PBSS_HD void sha256_suffix_block(const uint32_t (&d)[16], const uint32_t valid, const uint64_t len, const uint64_t off,
                                 const uint32_t (&key)[kSuffixWords], const bool last, uint32_t (&out)[16]) {
    // The key and the marker as nine words (the marker is the low byte of the ninth) start at byte ks of this block:
    // 0 .. 63 when the content ends here, -40 .. -1 when it ended in the block before (the key straddles, or only the marker or
    // only the length is left). In words: ks = 4 * kw + kr.
    const int32_t ks = (int32_t)((int64_t)len - (int64_t)off);
    const int32_t kw = ks >> 2;  // (arithmetic shift: the floor)
    const uint32_t kr = (uint32_t)ks & 3u;
    // A[i] = what lies at block word i - 10; the nine words move up by kw + 10 = 0 .. 25 words, one stage per bit of the
    // distance: no word of A is ever indexed by a run-time value, so everything stays in registers
    constexpr int kLow = 10, kN = 16 + kLow;
    uint32_t A[kN];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < kN; ++i) A[i] = i < (int)kSuffixWords ? key[i] : (i == (int)kSuffixWords ? 0x80u : 0u);
    const uint32_t s = (uint32_t)(kw + kLow);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int m = 1; m <= 16; m <<= 1) {
        const bool mv = (s & (uint32_t)m) != 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = kN - 1; i >= 0; --i) {
            const uint32_t from = i >= m ? A[i - m] : 0u;
            A[i] = mv ? from : A[i];
        }
    }
    const uint32_t up = 8u * kr, down = 32u - up;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 16; ++j) {
        const int32_t k = (int32_t)valid - 4 * j;  // data bytes in this word
        const uint32_t mask = k >= 4 ? 0xffffffffu : (k <= 0 ? 0u : ((1u << (8 * k)) - 1u));
        const uint32_t hi = A[j + kLow], lo = A[j + kLow - 1];
        const uint32_t kpart = kr ? ((hi << up) | (lo >> down)) : hi;
        out[j] = (d[j] & mask) | kpart;
    }
    if (last) {  // big-endian bit length in bytes 56 .. 63
        const uint64_t bits = (len + kSuffixBytes) * 8u;
        out[14] = bswap32((uint32_t)(bits >> 32));
        out[15] = bswap32((uint32_t)bits);
    }
}

}  // namespace pbss
