// The tail of the keyed chunk digest SHA-256(content || key) (pbs_plus_amd/csrc/sha256_suffix.h), as a CPU program built with
// -fsanitize=address,undefined by tests/test_sha256_suffix_native.py. For every length 0..200 (and 4096, 65535, 65536, 65537)
// at every start alignment 0..3 it assembles each tail block's data words the way the kernels do (aligned dword loads from a
// 4-byte-aligned buffer, the index clamped to the last dword that holds a valid byte, a funnel shift), calls
// pbss::sha256_suffix_block, and
//   * compares the block byte for byte with the padding of content || key built by the definition;
//   * runs a plain SHA-256 compression over all blocks and prints "digest <len> <align> <hex>".
// Prints "blocks ok <count>" or "blocks FAIL ...", and "sha256-suffix-ok". The buffer is a heap block of exactly the dwords
// that hold the content: AddressSanitizer sees any load beyond them.
#include "../../pbs_plus_amd/csrc/sha256_suffix.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

int g_fail = 0;

// tests/test_sha256_suffix_native.py: pattern(n, seed)
uint8_t pattern_byte(size_t i, uint32_t seed) {
    const uint32_t x = (uint32_t)(((uint64_t)i + (uint64_t)seed * 7919u) * 2654435761ull);
    return (uint8_t)((x >> 24) ^ (x >> 9));
}

const uint32_t kK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// one block of sixteen RAW little-endian words
void compress(uint32_t (&H)[8], const uint32_t (&raw)[16]) {
    uint32_t W[64];
    for (int i = 0; i < 16; ++i) W[i] = pbss::bswap32(raw[i]);
    for (int i = 16; i < 64; ++i) {
        const uint32_t s0 = rotr(W[i - 15], 7) ^ rotr(W[i - 15], 18) ^ (W[i - 15] >> 3);
        const uint32_t s1 = rotr(W[i - 2], 17) ^ rotr(W[i - 2], 19) ^ (W[i - 2] >> 10);
        W[i] = W[i - 16] + s0 + W[i - 7] + s1;
    }
    uint32_t a = H[0], b = H[1], c = H[2], d = H[3], e = H[4], f = H[5], g = H[6], h = H[7];
    for (int i = 0; i < 64; ++i) {
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kK[i] + W[i];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    H[0] += a; H[1] += b; H[2] += c; H[3] += d; H[4] += e; H[5] += f; H[6] += g; H[7] += h;
}

// The kernels' assembly of a block's data words: `buf` is 4-byte aligned, the chunk starts `align` bytes into it. Dword j of
// the block is loaded at min(j, the last dword that holds a valid byte), so nothing beyond the chunk's last dword is touched.
void data_words(const uint32_t *buf, uint32_t align, uint64_t off, uint32_t valid, uint32_t (&d)[16]) {
    uint32_t q[17];
    for (int j = 0; j < 17; ++j) q[j] = 0;
    uint32_t o = 0;
    if (valid) {
        const uint64_t p = align + off;
        o = (uint32_t)(p & 3u);
        const uint32_t *a = buf + (p - o) / 4;
        const uint32_t jmax = (o + valid - 1u) >> 2;
        for (uint32_t j = 0; j < 17; ++j) q[j] = a[j < jmax ? j : jmax];
    }
    const uint32_t sh = o * 8u;
    for (int j = 0; j < 16; ++j) d[j] = sh ? ((q[j] >> sh) | (q[j + 1] << (32u - sh))) : q[j];
}

bool one(uint64_t len, uint32_t align, const uint8_t (&key)[32], uint64_t *nblocks) {
    bool ok = true;
    // the chunk in exactly the dwords that hold it
    const size_t words = (size_t)((align + len + 3) / 4);
    uint32_t *buf = (uint32_t *)std::malloc(words ? words * 4 : 1);
    std::memset(buf, 0xA5, words * 4);
    uint8_t *bytes = (uint8_t *)buf + align;
    for (uint64_t i = 0; i < len; ++i) bytes[i] = pattern_byte((size_t)i, (uint32_t)len);
    // the definition: content || key || 0x80 || zeros || bit length, a multiple of 64 bytes
    std::vector<uint8_t> msg(bytes, bytes + len);
    msg.insert(msg.end(), key, key + 32);
    const uint64_t bits = (uint64_t)msg.size() * 8;
    msg.push_back(0x80);
    while (msg.size() % 64 != 56) msg.push_back(0);
    for (int k = 7; k >= 0; --k) msg.push_back((uint8_t)(bits >> (8 * k)));
    const uint64_t nblk = pbss::sha256_blocks(len, pbss::kSuffixBytes);
    if (nblk * 64 != msg.size()) {
        std::printf("  FAIL len %llu: %llu blocks, the definition has %zu bytes\n", (unsigned long long)len, (unsigned long long)nblk, msg.size());
        ok = false;
    }
    uint32_t kw[8];
    std::memcpy(kw, key, 32);
    uint32_t H[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    for (uint64_t blk = 0; ok && blk < nblk; ++blk) {
        const uint64_t off = blk * 64;
        uint32_t raw[16];
        if (off + 64 <= len) {  // a pure data block: the kernels' other path
            data_words(buf, align, off, 64, raw);
        } else {
            const uint32_t valid = len > off ? (uint32_t)(len - off) : 0u;
            uint32_t d[16];
            data_words(buf, align, off, valid, d);
            pbss::sha256_suffix_block(d, valid, len, off, kw, blk + 1 == nblk, raw);
            ++*nblocks;
        }
        if (std::memcmp(raw, msg.data() + off, 64) != 0) {
            if (g_fail++ < 20) std::printf("  FAIL len %llu align %u block %llu differs from the definition\n", (unsigned long long)len, align, (unsigned long long)blk);
            ok = false;
        }
        compress(H, raw);
    }
    std::printf("digest %llu %u ", (unsigned long long)len, align);
    for (int j = 0; j < 8; ++j) std::printf("%08x", H[j]);
    std::printf("\n");
    std::free(buf);
    return ok;
}

}  // namespace

int main() {
    uint8_t key[32];
    for (int i = 0; i < 32; ++i) key[i] = pattern_byte((size_t)i, 0x4b45u);
    bool ok = true;
    uint64_t nblocks = 0;
    std::vector<uint64_t> lens;
    for (uint64_t l = 0; l <= 200; ++l) lens.push_back(l);
    for (uint64_t l : {4096ull, 65535ull, 65536ull, 65537ull}) lens.push_back(l);
    for (uint64_t l : lens)
        for (uint32_t a = 0; a < 4; ++a) ok = one(l, a, key, &nblocks) && ok;
    if (ok) std::printf("blocks ok %llu\n", (unsigned long long)nblocks);
    else std::printf("blocks FAIL\n");
    if (ok) std::printf("sha256-suffix-ok\n");
    return ok ? 0 : 1;
}
