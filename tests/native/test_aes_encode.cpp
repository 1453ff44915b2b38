// What pbsgpu_blob_encode3_device rests on, as a CPU program built with -fsanitize=address,undefined by
// tests/test_aes_encode_native.py: aes_gcm.h's piece walk run IN PLACE (in == out, the way k_aese_pieces encrypts a frame
// where it lies), and the host plan's additions in blob_plan.h (slot offsets for either header size, the piece table for the
// slots' capacities, the duplicate-IV check, the statistics).
// Prints one line per section, "<section> ok <count>" or "<section> FAIL ...", and "aes-encode-ok".
// Every buffer is a heap block of exactly guard + length + guard bytes; the guards are checked after every call and
// AddressSanitizer watches everything beyond them.
#include "../../pbs_plus_amd/csrc/aes_gcm.h"
#include "../../pbs_plus_amd/csrc/blob_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    for (size_t i = 0; i < n; ++i) {
        const uint32_t x = (uint32_t)(((uint64_t)i + (uint64_t)seed * 7919u) * 2654435761ull);
        v[i] = (uint8_t)((x >> 24) ^ (x >> 9));
    }
    return v;
}

struct Guarded {  // exactly guard + n + guard bytes
    uint8_t *base;
    size_t n;
    explicit Guarded(size_t len) : base((uint8_t *)std::malloc(len + 2 * kGuard)), n(len) { std::memset(base, kGuardByte, len + 2 * kGuard); }
    Guarded(const uint8_t *src, size_t len) : Guarded(len) {
        if (len) std::memcpy(p(), src, len);
    }
    ~Guarded() { std::free(base); }
    Guarded(const Guarded &) = delete;
    uint8_t *p() { return base + kGuard; }
    bool intact() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (base[i] != kGuardByte || base[kGuard + n + i] != kGuardByte) return false;
        return true;
    }
};

void report(const char *name, bool ok, long count) { std::printf("%s %s %ld\n", name, ok ? "ok" : "FAIL", count); }

// encrypting in place = encrypting to a second buffer = the serial definition; decrypting in place gives the message back
bool in_place(const KeyTables &kt, uint32_t n, uint32_t seed) {
    bool ok = true;
    const std::vector<uint8_t> plain = pattern(n, seed), iv = pattern(16, 900 + seed);
    Guarded src(plain.data(), n), apart(n), serial(n), same(plain.data(), n);
    uint8_t t1[16], t2[16], t3[16], t4[16];
    CHECK(crypt_by_pieces(kt, iv.data(), 16, src.p(), apart.p(), n, true, t1) == OK, "apart, len %u", n);
    crypt_serial(kt, iv.data(), 16, src.p(), serial.p(), n, true, t2);
    CHECK(crypt_by_pieces(kt, iv.data(), 16, same.p(), same.p(), n, true, t3) == OK, "in place, len %u", n);
    CHECK(std::memcmp(t1, t2, 16) == 0 && std::memcmp(t1, t3, 16) == 0, "tags differ, len %u", n);
    CHECK(std::memcmp(apart.p(), serial.p(), n) == 0, "by pieces != serial, len %u", n);
    CHECK(std::memcmp(apart.p(), same.p(), n) == 0, "in place != apart, len %u", n);
    CHECK(std::memcmp(src.p(), plain.data(), n) == 0, "the source of the run with two buffers was written, len %u", n);
    std::memcpy(t4, t3, 16);
    CHECK(crypt_by_pieces(kt, iv.data(), 16, same.p(), same.p(), n, false, t4) == OK, "the tag of the in-place run, len %u", n);
    CHECK(std::memcmp(same.p(), plain.data(), n) == 0, "decrypt in place, len %u", n);
    CHECK(src.intact() && apart.intact() && serial.intact() && same.intact(), "guard bytes, len %u", n);
    return ok;
}

pbsgpu_segment seg(uint64_t off, uint64_t len) {
    pbsgpu_segment s;
    s.offset = off;
    s.length = len;
    return s;
}

bool offsets_section(long *count) {
    bool ok = true;
    const uint64_t lens[] = {0, 1, 15, 16, 17, 4095, 65535, 65536, 65537, 3 * 65536 + 5, 1, 0, 300000};
    std::vector<pbsgpu_segment> segs;
    for (uint64_t l : lens) segs.push_back(seg(7 * segs.size(), l));
    const uint32_t n = (uint32_t)segs.size();
    for (uint32_t hdr : {(uint32_t)PBSGPU_BLOB_HEADER_SIZE, (uint32_t)PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE}) {
        Guarded o((n + 1) * 8);
        uint64_t total = 1, sized = 2;
        CHECK(pbsp::slot_offsets(segs.data(), n, hdr, (uint64_t *)o.p(), &total), "slot_offsets, header %u", hdr);
        CHECK(pbsp::slot_offsets(segs.data(), n, hdr, nullptr, &sized) && sized == total, "without offsets, header %u", hdr);
        uint64_t at = 0;
        for (uint32_t i = 0; i < n; ++i) {  // by the definition: back to back, header + length each
            uint64_t got;
            std::memcpy(&got, o.p() + 8 * i, 8);
            CHECK(got == at, "offsets[%u] = %llu, want %llu (header %u)", i, (unsigned long long)got, (unsigned long long)at, hdr);
            at += hdr + lens[i];
            ++*count;
        }
        uint64_t last;
        std::memcpy(&last, o.p() + 8 * n, 8);
        CHECK(last == at && total == at && o.intact(), "the total, header %u", hdr);
        CHECK(hdr == 12 || hdr == 44, "the header sizes");
    }
    uint64_t total = 0;
    CHECK(pbsp::slot_offsets(nullptr, 0, 44, nullptr, &total) && total == 0, "no chunk");
    const pbsgpu_segment huge[2] = {seg(0, ~0ull - 50), seg(0, 100)};
    CHECK(pbsp::slot_offsets(huge, 1, 44, nullptr, &total) && total == huge[0].length + 44, "the largest sum that fits");
    CHECK(!pbsp::slot_offsets(huge, 2, 44, nullptr, &total), "the sum wraps");
    const pbsgpu_segment wrap1 = seg(0, ~0ull - 10);
    CHECK(!pbsp::slot_offsets(&wrap1, 1, 44, nullptr, &total), "length + header wraps");
    *count += 4;
    return ok;
}

// the table planned for the capacities against a loop by the definition; and what a kernel does with a real length below it
bool pieces_section(long *count) {
    bool ok = true;
    const uint64_t lens[] = {0, 1, 65535, 65536, 65537, 3 * 65536 + 5, 300000, 17, 0, 2 * 65536};
    std::vector<pbsgpu_segment> segs;
    for (uint64_t l : lens) segs.push_back(seg(0, l));
    pbsp::PieceTable t;
    CHECK(pbsp::capacity_pieces(segs.data(), (uint32_t)segs.size(), t), "capacity_pieces");
    uint64_t p = 0;
    for (uint32_t i = 0; i < segs.size(); ++i) {
        CHECK(t.pbase[i] == p, "pbase[%u]", i);
        for (uint64_t at = 0; at < lens[i]; at += 65536, ++p) {  // one piece per started 64 KiB
            CHECK(p < t.owner.size() && t.owner[p] == i, "owner[%llu]", (unsigned long long)p);
            ++*count;
        }
        CHECK(pbsa::pieces_of((uint32_t)lens[i]) == p - t.pbase[i], "the cipher's count of pieces, length %llu", (unsigned long long)lens[i]);
        // a message shorter than the capacity (a frame that won): the planned pieces at or beyond pieces_of(real) are
        // skipped, the others cover exactly `real` bytes
        for (uint64_t real : {(uint64_t)0, (uint64_t)1, lens[i] / 3, lens[i] - (lens[i] ? 1 : 0), lens[i]}) {
            if (real > lens[i]) continue;
            uint64_t covered = 0;
            for (uint32_t k = 0; k < p - t.pbase[i]; ++k) {
                if (k >= pbsa::pieces_of((uint32_t)real)) continue;
                const uint32_t pl = pbsa::piece_len((uint32_t)real, k);
                CHECK(pl >= 1 && pl <= kPiece, "piece_len(%llu, %u) = %u", (unsigned long long)real, k, pl);
                covered += pl;
            }
            CHECK(covered == real, "pieces of %llu cover %llu", (unsigned long long)real, (unsigned long long)covered);
            ++*count;
        }
    }
    CHECK(t.pbase[segs.size()] == p && t.np == p && t.owner.size() == p, "the piece count");
    return ok;
}

bool ivs_section(long *count) {
    bool ok = true;
    const uint32_t n = 200;
    std::vector<uint8_t> ivs;
    for (uint32_t i = 0; i < n; ++i) {
        const std::vector<uint8_t> v = pattern(16, 5000 + i);
        ivs.insert(ivs.end(), v.begin(), v.end());
    }
    Guarded g(ivs.data(), ivs.size());
    CHECK(pbsp::ivs_distinct(g.p(), n), "distinct IVs refused");
    CHECK(pbsp::ivs_distinct(g.p(), 1) && pbsp::ivs_distinct(g.p(), 0) && pbsp::ivs_distinct(nullptr, 0), "none and one");
    *count += 2;
    const uint32_t pairs[][2] = {{0, 1}, {0, n - 1}, {n - 2, n - 1}, {17, 93}, {93, 17}};
    for (const auto &pr : pairs) {
        Guarded d(ivs.data(), ivs.size());
        std::memcpy(d.p() + 16 * pr[1], d.p() + 16 * pr[0], 16);
        CHECK(!pbsp::ivs_distinct(d.p(), n), "IV %u = IV %u not seen", pr[0], pr[1]);
        for (int byte : {0, 7, 8, 15}) {  // one differing byte anywhere is enough
            d.p()[16 * pr[1] + byte] ^= 0x80;
            CHECK(pbsp::ivs_distinct(d.p(), n), "IVs that differ in byte %d taken for equal", byte);
            d.p()[16 * pr[1] + byte] ^= 0x80;
            ++*count;
        }
        CHECK(d.intact(), "guard bytes");
        ++*count;
    }
    Guarded z(32);  // two all-zero IVs
    std::memset(z.p(), 0, 32);
    CHECK(!pbsp::ivs_distinct(z.p(), 2), "two zero IVs");
    CHECK(std::memcmp(g.p(), ivs.data(), ivs.size()) == 0 && g.intact(), "the caller's IVs were reordered");
    *count += 2;
    return ok;
}

bool stats_section(long *count) {
    bool ok = true;
    pbsgpu_encode_stats3 st;
    std::memset(&st, 0, sizeof(st));
    pbsp::count_blob3(st, PBSGPU_BLOB_UNCOMPRESSED, 12 + 100, 100);
    pbsp::count_blob3(st, PBSGPU_BLOB_COMPRESSED, 12 + 40, 100);
    pbsp::count_blob3(st, PBSGPU_BLOB_ENCRYPTED, 44 + 100, 100);
    pbsp::count_blob3(st, PBSGPU_BLOB_ENCRYPTED_COMPRESSED, 44 + 30, 100);
    pbsp::count_blob3(st, PBSGPU_BLOB_ENCRYPTED, 44, 0);
    CHECK(st.blobs[0] == 1 && st.blobs[1] == 1 && st.blobs[2] == 2 && st.blobs[3] == 1, "blobs");
    CHECK(st.blob_bytes[0] == 112 && st.blob_bytes[1] == 52 && st.blob_bytes[2] == 188 && st.blob_bytes[3] == 74, "blob_bytes");
    CHECK(st.chunk_bytes[0] == 100 && st.chunk_bytes[1] == 100 && st.chunk_bytes[2] == 100 && st.chunk_bytes[3] == 100, "chunk_bytes");
    CHECK(st.frame_bytes == 70 && st.crc_bytes == 270 && st.aes_bytes == 130, "frame, crc, aes bytes");
    CHECK(sizeof(pbsgpu_encode_stats3) == 15 * 8, "the layout of pbsgpu_encode_stats3");
    *count += 5;
    return ok;
}

}  // namespace

int main() {
    KeyTables *kt = new KeyTables();
    const std::vector<uint8_t> key = pattern(32, 2005);
    make_key(key.data(), *kt);
    bool all = true;
    {
        bool ok = true;
        long count = 0;
        const uint32_t lens[] = {1, 15, 16, 17, 4095, 65535, 65536, 65537, 3 * 65536 + 5};
        for (uint32_t n : lens) {
            ok = in_place(*kt, n, n % 97) && ok;
            ++count;
        }
        report("in-place", ok, count);
        all = all && ok;
    }
    struct {
        const char *name;
        bool (*fn)(long *);
    } sections[] = {{"offsets", offsets_section}, {"pieces", pieces_section}, {"ivs", ivs_section}, {"stats", stats_section}};
    for (auto &s : sections) {
        long count = 0;
        const bool ok = s.fn(&count);
        report(s.name, ok, count);
        all = all && ok;
    }
    delete kt;
    if (all && g_fail == 0) std::printf("aes-encode-ok\n");
    return all && g_fail == 0 ? 0 : 1;
}
