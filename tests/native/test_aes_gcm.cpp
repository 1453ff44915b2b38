// aes_gcm.h (pbs_plus_amd/csrc) as a CPU program, built with -fsanitize=address,undefined by tests/test_aes_gcm_native.py.
//   test_aes_gcm <cases>      cases: one line per golden case, "keyhex ivhex len seed taghex crc32" (ivhex "-" = empty)
// Prints one line per section, "<section> ok <count>" or "<section> FAIL ...", the coverage word, and "aes-gcm-ok".
// Every output buffer is a heap block of exactly guard + length + guard bytes; the guards are checked after every call and
// AddressSanitizer watches everything beyond them.
#define PBSGPU_AES_COVERAGE 1
#include "../../pbs_plus_amd/csrc/aes_gcm.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace pbsa;

namespace {

constexpr size_t kGuard = 32;
constexpr uint8_t kGuardByte = 0xA5;
int g_fail = 0;

#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (g_fail++ < 20) {          \
                std::printf("  FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
            ok = false;                   \
        }                                 \
    } while (0)

// tests/aes_inputs.py: pattern(n, seed)
std::vector<uint8_t> pattern(size_t n, uint32_t seed) {
    std::vector<uint8_t> v(n);
    if (seed == 0xffffffffu) return v;  // ZEROS
    for (size_t i = 0; i < n; ++i) {
        const uint32_t x = (uint32_t)(((uint64_t)i + (uint64_t)seed * 7919u) * 2654435761ull);
        v[i] = (uint8_t)((x >> 24) ^ (x >> 9));
    }
    return v;
}

uint32_t crc32(const uint8_t *p, size_t n) {
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = c >> 1 ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return v;
}

struct Guarded {  // exactly guard + n + guard bytes
    uint8_t *base;
    size_t n;
    explicit Guarded(size_t len) : base((uint8_t *)std::malloc(len + 2 * kGuard)), n(len) { std::memset(base, kGuardByte, len + 2 * kGuard); }
    ~Guarded() { std::free(base); }
    Guarded(const Guarded &) = delete;
    uint8_t *p() { return base + kGuard; }
    bool intact() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (base[i] != kGuardByte || base[kGuard + n + i] != kGuardByte) return false;
        return true;
    }
};

// an exact-size copy of the input, so that a read past it is seen
struct Exact {
    uint8_t *p;
    Exact(const uint8_t *src, size_t n) : p((uint8_t *)std::malloc(n ? n : 1)) {
        if (n) std::memcpy(p, src, n);
    }
    ~Exact() { std::free(p); }
    Exact(const Exact &) = delete;
};

// encrypt by pieces and by the definition, decrypt by pieces: everything agrees. Returns the tag and the ciphertext's CRC.
bool round_trip(const KeyTables &kt, const std::vector<uint8_t> &iv, const std::vector<uint8_t> &plain, uint8_t tag[16], uint32_t *crc) {
    bool ok = true;
    const uint32_t n = (uint32_t)plain.size();
    Exact in(plain.data(), n), ivx(iv.data(), iv.size());
    Guarded c1(n), c2(n), back(n);
    uint8_t t2[16];
    CHECK(crypt_by_pieces(kt, ivx.p, (uint32_t)iv.size(), in.p, c1.p(), n, true, tag) == OK, "encrypt status");
    crypt_serial(kt, ivx.p, (uint32_t)iv.size(), in.p, c2.p(), n, true, t2);
    CHECK(std::memcmp(tag, t2, 16) == 0, "tag by pieces != serial, len %u iv %zu", n, iv.size());
    CHECK(n == 0 || std::memcmp(c1.p(), c2.p(), n) == 0, "ciphertext by pieces != serial, len %u", n);
    Exact ct(c1.p(), n);
    uint8_t t3[16];
    std::memcpy(t3, tag, 16);
    CHECK(crypt_by_pieces(kt, ivx.p, (uint32_t)iv.size(), ct.p, back.p(), n, false, t3) == OK, "decrypt status, len %u", n);
    CHECK(n == 0 || std::memcmp(back.p(), plain.data(), n) == 0, "decrypt(encrypt(x)) != x, len %u", n);
    CHECK(c1.intact() && c2.intact() && back.intact(), "guard bytes, len %u", n);
    *crc = crc32(c1.p(), n);
    return ok;
}

void report(const char *name, bool ok, long count) { std::printf("%s %s %ld\n", name, ok ? "ok" : "FAIL", count); }

bool same(Blk a, Blk b) { return std::memcmp(&a, &b, 16) == 0; }

Blk rnd_blk(uint32_t seed) {
    const auto v = pattern(16, seed);
    return load_be(v.data());
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    // ---- the golden cases ----
    {
        bool ok = true;
        long count = 0, wraps = 0;
        FILE *f = std::fopen(argv[1], "r");
        if (!f) return 2;
        char key[80], iv[200], tag[40];
        unsigned len, seed, crc;
        while (std::fscanf(f, "%79s %199s %u %u %39s %u", key, iv, &len, &seed, tag, &crc) == 6) {
            KeyTables kt;
            make_key(unhex(key).data(), kt);
            const auto ivb = unhex(iv), want = unhex(tag);
            uint8_t got[16];
            uint32_t c = 0;
            CHECK(round_trip(kt, ivb, pattern(len, seed), got, &c), "case %ld", count);
            CHECK(std::memcmp(got, want.data(), 16) == 0, "case %ld (len %u): tag", count, len);
            CHECK(c == crc, "case %ld (len %u): ciphertext CRC %08x, recorded %08x", count, len, c, crc);
            const Blk j0 = j0_of(kt.h, ivb.data(), (uint32_t)ivb.size());
            const uint64_t blocks = ((uint64_t)len + 15) / 16;
            if ((uint64_t)j0.w[3] + blocks > 0xffffffffull) ++wraps;
            ++count;
        }
        std::fclose(f);
        report("golden", ok && count > 0, count);
        report("golden-wraps", ok, wraps);
    }
    uint8_t keyb[32];
    {
        const auto k = pattern(32, 77);
        std::memcpy(keyb, k.data(), 32);
    }
    KeyTables kt;
    make_key(keyb, kt);
    // ---- IV lengths 8, 12, 16, 60 x every length 0..49 ----
    {
        bool ok = true;
        long count = 0;
        for (uint32_t ivn : {8u, 12u, 16u, 60u})
            for (uint32_t n = 0; n < 50; ++n, ++count) {
                uint8_t t[16];
                uint32_t c;
                CHECK(round_trip(kt, pattern(ivn, 100 + n), pattern(n, n), t, &c), "iv %u len %u", ivn, n);
            }
        report("lengths", ok, count);
    }
    // ---- pieces + fold = the serial chain: 1, 2, 3 and 5 pieces with odd tails, and a whole number of pieces ----
    {
        bool ok = true;
        long count = 0;
        for (uint32_t n : {kPiece - 7, kPiece, kPiece + 1, 2 * kPiece + 5, 3 * kPiece - 16, 5 * kPiece + 33}) {
            uint8_t t[16];
            uint32_t c;
            CHECK(round_trip(kt, pattern(16, n), pattern(n, n), t, &c), "len %u", n);
            ++count;
        }
        report("pieces", ok, count);
    }
    // ---- every split of a short chain into three parts folds to the serial hash ----
    {
        bool ok = true;
        long count = 0;
        const uint32_t nb = 23;
        std::vector<Blk> c(nb);
        for (uint32_t i = 0; i < nb; ++i) c[i] = rnd_blk(500 + i);
        Blk serial{{0, 0, 0, 0}};
        for (uint32_t i = 0; i < nb; ++i) serial = ghash_step(serial, c[i], kt.h);
        auto partial = [&](uint32_t a, uint32_t b) {  // sum C_j H^(b-1-j), a <= j < b
            Blk y{{0, 0, 0, 0}};
            for (uint32_t j = a; j < b; ++j) y = bxor(mul(y, kt.h), c[j]);
            return y;
        };
        for (uint32_t a = 0; a <= nb; ++a)
            for (uint32_t b = a; b <= nb; ++b, ++count) {
                const uint32_t cut[4] = {0, a, b, nb};
                Blk terms{{0, 0, 0, 0}};
                for (int k = 0; k < 3; ++k)
                    if (cut[k] < cut[k + 1]) terms = bxor(terms, mul_pow(partial(cut[k], cut[k + 1]), nb - cut[k + 1] + 1, kt.pow2));
                CHECK(same(terms, serial), "split %u %u", a, b);
            }
        report("splits", ok, count);
    }
    // ---- H^n against repeated multiplication; the key's tables ----
    {
        bool ok = true;
        long count = 0;
        Blk p = gf_one();
        for (uint32_t n = 0; n <= 600; ++n, ++count) {
            CHECK(same(gf_pow(kt.h, n), p), "gf_pow %u", n);
            CHECK(same(mul_pow(gf_one(), n, kt.pow2), p), "mul_pow %u", n);
            if (n < kStride) CHECK(same(kt.low[n], p), "low %u", n);
            if (n == kStride) CHECK(same(kt.stride[0x80], p), "stride table");
            p = mul(p, kt.h);
        }
        for (uint64_t a : {4096ull, 65537ull, (1ull << 28) - 1, (1ull << 31) + 12345})
            for (uint64_t b : {1ull, 4095ull, 1ull << 20}) {
                CHECK(same(gf_pow(kt.h, a + b), mul(gf_pow(kt.h, a), gf_pow(kt.h, b))), "pow sum");
                CHECK(same(mul_pow(gf_one(), a + b, kt.pow2), gf_pow(kt.h, a + b)), "mul_pow large");
                ++count;
            }
        const Blk hs = gf_pow(kt.h, kStride);
        for (uint32_t i = 0; i < 300; ++i, ++count) {
            const Blk x = i < 256 ? Blk{{i < 128 ? 0x80000000u >> (i & 31) : 0, 0, 0, i >= 128 ? i - 128 : 0}} : rnd_blk(900 + i);
            CHECK(same(mul_tab(x, kt.stride, kt.red), mul(x, hs)), "mul_tab %u", i);
            CHECK(same(mul(x, hs), mul(hs, x)), "mul commutes %u", i);
        }
        report("powers", ok, count);
    }
    // ---- a 33-byte message: every single-bit flip of ciphertext, tag and IV is BAD_TAG, and the output is zero ----
    {
        bool ok = true;
        long count = 0;
        const auto plain = pattern(33, 5), iv = pattern(16, 6);
        Guarded ct(33);
        uint8_t tag[16];
        crypt_by_pieces(kt, iv.data(), 16, plain.data(), ct.p(), 33, true, tag);
        for (uint32_t bit = 0; bit < (33 + 16 + 16) * 8; ++bit, ++count) {
            std::vector<uint8_t> c(ct.p(), ct.p() + 33), t(tag, tag + 16), v(iv);
            uint8_t *where = bit < 264 ? &c[bit / 8] : bit < 264 + 128 ? &t[(bit - 264) / 8] : &v[(bit - 392) / 8];
            *where ^= (uint8_t)(1u << (bit & 7));
            Exact cx(c.data(), 33), vx(v.data(), 16);
            Guarded out(33);
            CHECK(crypt_by_pieces(kt, vx.p, 16, cx.p, out.p(), 33, false, t.data()) == BAD_TAG, "bit %u accepted", bit);
            bool zero = true;
            for (uint32_t i = 0; i < 33; ++i) zero = zero && out.p()[i] == 0;
            CHECK(zero && out.intact(), "bit %u: output", bit);
        }
        Guarded out(33);
        CHECK(crypt_by_pieces(kt, iv.data(), 16, ct.p(), out.p(), 33, false, tag) == OK, "unflipped");
        CHECK(std::memcmp(out.p(), plain.data(), 33) == 0, "unflipped bytes");
        report("flips", ok, count);
    }
    std::printf("coverage %llx of %d\n", (unsigned long long)g_cov, (int)A_NBITS);
    if (g_fail) return 1;
    std::printf("aes-gcm-ok\n");
    return 0;
}
