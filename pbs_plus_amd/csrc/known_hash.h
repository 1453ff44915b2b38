// The hash of the known-chunk set (known.hip): the mix, the home-slot hash, the tag and the 32-bit sort key
// of a digest. One copy for the kernels and for host code: without hipcc the functions are plain inline C++, so
// tests/native/test_known_hash.cpp prints what the device computes and tests/known_inputs.py crafts digests against it.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define PBSK_HD __host__ __device__ __forceinline__
#else
#define PBSK_HD inline
#endif

namespace pbsk {

PBSK_HD uint64_t known_mix(uint64_t x) {  // splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// home-slot hash from digest bytes 8..31
PBSK_HD uint64_t known_home(const uint64_t w[4]) {
    return known_mix(w[1] ^ known_mix(w[2] ^ known_mix(w[3])));
}

PBSK_HD uint64_t known_tag(uint64_t w0) { return w0 ? w0 : 1ull; }

// digest i of a record array (stride 48) or of .didx entries (stride 40): both keep it at offset 8, 8-byte aligned
PBSK_HD void known_load(const uint8_t *base, uint32_t stride, uint64_t i, uint64_t w[4]) {
    const uint64_t *q = reinterpret_cast<const uint64_t *>(base + i * stride + 8);
    w[0] = q[0];
    w[1] = q[1];
    w[2] = q[2];
    w[3] = q[3];
}

// 32-bit sort key: a mix of all 32 digest bytes (h = known_home(w))
PBSK_HD uint32_t known_key(uint64_t h, const uint64_t w[4]) { return (uint32_t)known_mix(h ^ w[0]); }

}  // namespace pbsk
