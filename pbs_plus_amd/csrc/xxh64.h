// XXH64 with a seed (the content checksum of a zstd frame is its low 32 bits, seed 0; RFC 8878 §3.1.1): ONE
// implementation, compiled twice, in the manner of zstd_decode.h. Under hipcc every function is __host__ __device__;
// without hipcc it is plain inline C++, and that build is what tests/native/test_zstd_checksum.cpp runs under
// AddressSanitizer. No HIP and no libc beyond the fixed-width integers.
//
// The four accumulators of the stripe loop are four independent serial chains, so FOUR LANES carry one range: lane j
// (P::lane() < 4) takes word j of every 32-byte stripe. They leave their accumulators in `box`, and after P::sync() the
// first lane merges them, walks the tail (steps of 8, 4 and 1 bytes) and runs the avalanche; after a second P::sync()
// every lane reads the result. A policy with one lane (the host) does all four chains itself. Lanes beyond the fourth
// only take part in the syncs. The policy is that of zstd_decode.h: P::lane(), P::lanes(), P::sync(), P::uni().
//
// Every lane calls xxh64 with the same arguments of ITS range and reaches both syncs whatever the range's length: the
// stripe loop is the only part whose trip count depends on the length, and it holds no sync. So lanes that carry ranges
// of different lengths may call it together (k_xxh64_ranges: sixteen ranges per wave).
//
// Loads: eight bytes at a time at any alignment through __builtin_memcpy (gfx950 loads unaligned words from global
// memory); the pointer comes from a kernel argument, so they are global_* loads.
#pragma once

#include <cstdint>

#include "zstd_decode.h"  // PBSZ_HD, the lane policy

#ifdef PBSGPU_ZSTD_COVERAGE  // CPU test build only: the branches of xxh64.h and of the checksum and stream paths of the
namespace pbsz {             // two format cores, a bitmap of their own (names: tests/native/test_zstd_checksum.cpp)
inline uint64_t g_cov2 = 0;
}
#define PBSZ_COV2(bit) (::pbsz::g_cov2 |= 1ull << (bit))
#else
#define PBSZ_COV2(bit) ((void)0)
#endif

namespace pbsz {

enum : int {  // coverage bits of the second bitmap
    K_XXH_STRIPES, K_XXH_SHORT, K_XXH_TAIL_8, K_XXH_TAIL_4, K_XXH_TAIL_1, K_XXH_EMPTY,
    K_SUM_GOOD, K_SUM_BAD, K_SUM_ABSENT, K_SUM_NOT_ASKED,
    K_ONE_FRAME, K_STREAM_EMPTY, K_STREAM_FRAME, K_STREAM_SECOND_FRAME, K_STREAM_SKIPPABLE, K_STREAM_SKIPPABLE_CUT,
    K_STREAM_SHORT_TAIL, K_STREAM_FRAME_FAILS, K_STREAM_NO_FRAME,
    K_ENC_SUM, K_ENC_NO_SUM, K_ENC_SUM_NO_ROOM,
    K_NBITS
};

namespace xxh {

constexpr uint64_t kP1 = 0x9E3779B185EBCA87ull, kP2 = 0xC2B2AE3D27D4EB4Full, kP3 = 0x165667B19E3779F9ull,
                   kP4 = 0x85EBCA77C2B2AE63ull, kP5 = 0x27D4EB2F165667C5ull;

PBSZ_HD uint64_t rotl(uint64_t x, int r) { return x << r | x >> (64 - r); }
PBSZ_HD uint64_t rd64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
PBSZ_HD uint32_t rd32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
PBSZ_HD uint64_t rnd(uint64_t acc, uint64_t w) { return rotl(acc + w * kP2, 31) * kP1; }
PBSZ_HD uint64_t merge(uint64_t h, uint64_t acc) { return (h ^ rnd(0, acc)) * kP1 + kP4; }

// accumulator j (0..3) over the `stripes` whole 32-byte stripes at p: the serial chain of one lane
PBSZ_HD uint64_t chain(const uint8_t *p, uint64_t stripes, uint64_t seed, uint32_t j) {
    uint64_t acc = j == 0 ? seed + kP1 + kP2 : j == 1 ? seed + kP2 : j == 2 ? seed : seed - kP1;
    const uint8_t *q = p + 8 * j;
    uint64_t s = 0;
    for (; s + 8 <= stripes; s += 8, q += 256) {  // eight loads in flight: one at a time, the chain waits for memory
        uint64_t w[8];
        for (int k = 0; k < 8; ++k) w[k] = rd64(q + 32 * k);
        for (int k = 0; k < 8; ++k) acc = rnd(acc, w[k]);
    }
    for (; s < stripes; ++s, q += 32) acc = rnd(acc, rd64(q));
    return acc;
}

// the rest, on one lane: v = the four accumulators (unused below 32 bytes)
PBSZ_HD uint64_t finish(const uint64_t *v, const uint8_t *p, uint64_t n, uint64_t seed) {
    uint64_t h;
    if (n >= 32) {
        PBSZ_COV2(K_XXH_STRIPES);
        h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18);
        h = merge(h, v[0]);
        h = merge(h, v[1]);
        h = merge(h, v[2]);
        h = merge(h, v[3]);
    } else {
        PBSZ_COV2(n ? K_XXH_SHORT : K_XXH_EMPTY);
        h = seed + kP5;
    }
    h += n;
    uint64_t i = n & ~31ull;
    for (; n - i >= 8; i += 8) {
        PBSZ_COV2(K_XXH_TAIL_8);
        h = rotl(h ^ rnd(0, rd64(p + i)), 27) * kP1 + kP4;
    }
    if (n - i >= 4) {
        PBSZ_COV2(K_XXH_TAIL_4);
        h = rotl(h ^ rd32(p + i) * kP1, 23) * kP2 + kP3;
        i += 4;
    }
    for (; i < n; ++i) {
        PBSZ_COV2(K_XXH_TAIL_1);
        h = rotl(h ^ p[i] * kP5, 11) * kP1;
    }
    h ^= h >> 33;
    h *= kP2;
    h ^= h >> 29;
    h *= kP3;
    h ^= h >> 32;
    return h;
}

}  // namespace xxh

// XXH64 of p[0, n) with `seed`, on every lane. box: five words that the lanes of this range share (LDS in a kernel) and
// nobody else touches between the call's first sync and its return. Loads only inside p[0, n).
template <class P>
PBSZ_HD uint64_t xxh64(const uint8_t *p, uint64_t n, uint64_t seed, uint64_t *box) {
    const uint32_t lane = (uint32_t)P::lane();
    const uint64_t stripes = n >> 5;
    if (P::lanes() >= 4) {
        if (lane < 4) box[lane] = xxh::chain(p, stripes, seed, lane);
    } else {
        for (uint32_t j = 0; j < 4; ++j) box[j] = xxh::chain(p, stripes, seed, j);
    }
    P::sync();
    if (lane == 0) box[4] = xxh::finish(box, p, n, seed);
    P::sync();
    const uint64_t h = box[4];
    P::sync();  // the box is free for the next call
    return h;
}

}  // namespace pbsz
