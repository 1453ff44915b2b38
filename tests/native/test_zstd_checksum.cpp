// The CPU build of pbs_plus_amd/csrc/xxh64.h, zstd_stream.h and the checksum of zstd_encode.h under AddressSanitizer +
// UBSan (tests/test_zstd_checksum_native.py): XXH64 of ranges at every alignment, libzstd frames with a checksum and whole
// streams through decode2 with their seeded single-byte mutations and truncations, and this project's own frames with and
// without the checksum in every encoder mode. Every input lies in an exact heap copy (so that ASan sees a read one byte
// past it), every output between two guards. One line per call goes to the results file, so that the Python side can set
// them against the golden file and, where it loads, against libzstd.
//
// usage: test_zstd_checksum <ops file> <results file> <frames file> <stride> <first>   (ops first, first + stride, ...)
// ops file: u32 count, then per op a u8 kind and
//   'X': u32 base, u64 seed, u64 n, n bytes            XXH64 of bytes [base, n)        -> "i X <hash>"
//   'D': u32 flags, u64 room, u32 nmut, u32 cuts, u64 n, n bytes   decode2              -> "i D 0 status decoded crc", then
//        "i M j status decoded crc" per mutation j < nmut (zstd_inputs.mutation(i, j, n)) and, with cuts, "i C len status
//        decoded crc" per truncation
//   'E': u32 mode (bit 0 tables, bit 1 window 17), u64 n, n bytes  encode_frame without and with the checksum
//        -> "i E status flen status_sum flen_sum status_small checks offset" (checks: bit 0 the frame with the checksum is
//        the frame without, bit 2 of byte 4 set, four bytes more; bit 1 decode2 with F_CHECKSUM gives the content back;
//        bit 2 its last four bytes are what xxh64.h says; offset: where the frame with the checksum lies in the frames file)
#define PBSGPU_ZSTD_COVERAGE 1
#include "../../pbs_plus_amd/csrc/zstd_encode.h"
#include "../../pbs_plus_amd/csrc/zstd_stream.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {

constexpr size_t kGuard = 64;
constexpr uint8_t kGuardByte = 0xa5;
namespace ze = pbsz::enc;

uint32_t crc_table[256];

void crc_init() {
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
        crc_table[i] = c;
    }
}

uint32_t crc32(const uint8_t *p, size_t n) {
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) c = crc_table[(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}

uint64_t splitmix(uint64_t x) {  // tests/zstd_inputs.py has the same three lines
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

pbsz::State g_state;
pbsz::Walk g_walk;
ze::State g_s;
ze::TState g_t;
ze::WState g_w;
ze::WTState g_wt;
std::vector<uint8_t> g_lit(pbsz::kLitMax + 2 * kGuard);
int g_failures = 0;

void fail(const char *what, size_t op) {
    std::printf("FAIL: op %zu: %s\n", op, what);
    ++g_failures;
}

uint64_t hash_of(const uint8_t *p, size_t n, uint64_t seed) {  // from an exact heap copy
    std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(copy.get(), p, n);
    uint64_t box[5];
    return pbsz::xxh64<pbsz::HostLanes>(copy.get(), n, seed, box);
}

int decode2(size_t op, const uint8_t *src_bytes, size_t n, size_t room, uint32_t flags, std::vector<uint8_t> &out, uint32_t *decoded) {
    std::vector<uint8_t> src(src_bytes, src_bytes + n);
    out.assign(room + 2 * kGuard, kGuardByte);
    std::memset(g_lit.data(), kGuardByte, kGuard);
    std::memset(g_lit.data() + kGuard + pbsz::kLitMax, kGuardByte, kGuard);
    const int st = pbsz::decode2<pbsz::HostLanes>(g_state, src.data(), (uint32_t)n, out.data() + kGuard, (uint32_t)room,
                                                  g_lit.data() + kGuard, flags, g_walk, decoded);
    for (size_t i = 0; i < kGuard; ++i)
        if (out[i] != kGuardByte || out[kGuard + room + i] != kGuardByte || g_lit[i] != kGuardByte ||
            g_lit[kGuard + pbsz::kLitMax + i] != kGuardByte) {
            fail("a guard byte was overwritten", op);
            break;
        }
    if (st < 0 || st > 4 || (st != pbsz::OK && *decoded != 0) || *decoded > room) fail("status or decoded out of range", op);
    return st;
}

int encode(uint32_t mode, const std::vector<uint8_t> &c, size_t room, bool sum, std::vector<uint8_t> &out, uint64_t *flen, size_t op) {
    const uint32_t n = (uint32_t)c.size();
    std::vector<uint8_t> blk(pbsz::kBlockMax), lit(pbsz::kBlockMax), src(c);
    std::vector<uint64_t> seqs(ze::kSeqCap);
    std::vector<uint32_t> tab(1u << ze::kWindowHashLog, 0xdeadbeefu);
    out.assign(room + 2 * kGuard, kGuardByte);
    uint8_t *dst = out.data() + kGuard;
    const uint64_t h = hash_of(c.data(), c.size(), 0);
    const uint64_t *hp = sum ? &h : nullptr;
    const ze::Src2 two{src.data(), src.data() + n, n};  // the window modes read a chunk in two parts: here it lies in one
    int st;
    switch (mode) {
    case 0: st = ze::encode_frame<ze::HostLanes>(g_s, (const uint8_t *)src.data(), n, dst, room, blk.data(), lit.data(), seqs.data(), flen, 0, nullptr, hp); break;
    case 1: st = ze::encode_frame<ze::HostLanes>(g_t, (const uint8_t *)src.data(), n, dst, room, blk.data(), lit.data(), seqs.data(), flen, 0, nullptr, hp); break;
    case 2: st = ze::encode_frame<ze::HostLanes>(g_w, two, n, dst, room, blk.data(), lit.data(), seqs.data(), flen, 17, tab.data(), hp); break;
    default: st = ze::encode_frame<ze::HostLanes>(g_wt, two, n, dst, room, blk.data(), lit.data(), seqs.data(), flen, 17, tab.data(), hp); break;
    }
    for (size_t i = 0; i < kGuard; ++i)
        if (out[i] != kGuardByte || out[kGuard + room + i] != kGuardByte) {
            fail("encode: a guard byte was overwritten", op);
            break;
        }
    return st;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const size_t stride = (size_t)std::atoi(argv[4]), first = (size_t)std::atoi(argv[5]);
    if (stride == 0) return 2;
    crc_init();
    FILE *f = std::fopen(argv[1], "rb");
    FILE *res = std::fopen(argv[2], "w");
    FILE *frames = std::fopen(argv[3], "wb");
    if (!f || !res || !frames) return 2;
    uint32_t count = 0;
    if (!read_exact(f, &count, 4)) return 2;
    std::vector<uint8_t> out, data;
    uint64_t dumped = 0;
    for (size_t op = 0; op < count; ++op) {
        uint8_t kind = 0;
        uint32_t a = 0, nmut = 0, cuts = 0;
        uint64_t seed = 0, room = 0, n = 0;
        if (!read_exact(f, &kind, 1) || !read_exact(f, &a, 4)) return 2;
        if (kind == 'X' && !read_exact(f, &seed, 8)) return 2;
        if (kind == 'D' && (!read_exact(f, &room, 8) || !read_exact(f, &nmut, 4) || !read_exact(f, &cuts, 4))) return 2;
        if (!read_exact(f, &n, 8)) return 2;
        data.resize(n);
        if (!read_exact(f, data.data(), n)) return 2;
        if (op % stride != first) continue;
        if (kind == 'X') {
            if (a > n) return 2;
            std::fprintf(res, "%zu X %016llx\n", op, (unsigned long long)hash_of(data.data() + a, n - a, seed));
        } else if (kind == 'D') {
            uint32_t decoded = 0;
            int st = decode2(op, data.data(), n, room, a, out, &decoded);
            std::fprintf(res, "%zu D 0 %d %u %u\n", op, st, decoded, crc32(out.data() + kGuard, decoded));
            for (uint64_t j = 0; j < nmut && n; ++j) {
                const uint64_t r = splitmix(((uint64_t)op << 32) + j + 77);
                const size_t at = r % n;
                const uint8_t old = data[at];
                data[at] = old ^ (uint8_t)(1 + (r >> 32) % 255);
                st = decode2(op, data.data(), n, room, a, out, &decoded);
                std::fprintf(res, "%zu M %llu %d %u %u\n", op, (unsigned long long)j, st, decoded, crc32(out.data() + kGuard, decoded));
                data[at] = old;
            }
            if (cuts) {
                std::vector<size_t> at;
                for (size_t l = 0; l <= 24 && l < n; ++l) at.push_back(l);
                for (size_t l = n > 12 ? n - 12 : 0; l < n; ++l) at.push_back(l);
                for (uint64_t j = 0; j < 40 && n; ++j) at.push_back(splitmix(op * 1000003ull + j) % n);
                for (size_t l : at) {
                    st = decode2(op, data.data(), l, room, a, out, &decoded);
                    std::fprintf(res, "%zu C %zu %d %u %u\n", op, l, st, decoded, crc32(out.data() + kGuard, decoded));
                }
            }
        } else if (kind == 'E') {
            const uint64_t bound = ze::encode_bound2(n, false), bound2 = ze::encode_bound2(n, true);
            std::vector<uint8_t> plain, sum;
            uint64_t flen0 = 0, flen1 = 0, flen2 = 0;
            const int st0 = encode(a, data, bound, false, plain, &flen0, op);
            const int st1 = encode(a, data, bound2, true, sum, &flen1, op);
            const int st2 = encode(a, data, bound2 - 1, true, out, &flen2, op);
            if (st2 != pbsz::OK && flen2 != 0) fail("a frame length without OK", op);
            unsigned checks = 0;
            if (st0 == pbsz::OK && st1 == pbsz::OK && flen1 == flen0 + 4) {
                const uint8_t *p = plain.data() + kGuard, *q = sum.data() + kGuard;
                bool same = (p[4] | 4u) == q[4] && !(p[4] & 4u) && std::memcmp(p, q, 4) == 0 && std::memcmp(p + 5, q + 5, flen0 - 5) == 0;
                if (same) checks |= 1u;
                uint32_t decoded = 0;
                std::vector<uint8_t> back;
                const int ds = decode2(op, q, flen1, n, pbsz::F_CHECKSUM, back, &decoded);
                if (ds == pbsz::OK && decoded == n && (n == 0 || std::memcmp(back.data() + kGuard, data.data(), n) == 0)) checks |= 2u;
                const uint32_t low = (uint32_t)hash_of(data.data(), n, 0);
                if (pbsz::load_le(q + flen1 - 4, 4) == low) checks |= 4u;
                // and the decoder refuses the same frame with one content byte of a raw block or one checksum byte changed
                std::vector<uint8_t> bad(q, q + flen1);
                bad[flen1 - 1] ^= 0x10;
                if (decode2(op, bad.data(), flen1, n, pbsz::F_CHECKSUM, back, &decoded) != pbsz::BAD_CHECKSUM) fail("a flipped checksum byte was taken", op);
                if (decode2(op, bad.data(), flen1, n, 0, back, &decoded) != pbsz::OK) fail("flags 0 verified a checksum", op);
            }
            std::fprintf(res, "%zu E %d %llu %d %llu %d %u %llu\n", op, st0, (unsigned long long)flen0, st1, (unsigned long long)flen1, st2,
                         checks, (unsigned long long)dumped);
            if (st1 == pbsz::OK) {
                std::fwrite(sum.data() + kGuard, 1, flen1, frames);
                dumped += flen1;
            }
        } else {
            return 2;
        }
    }
    std::fclose(f);
    std::fclose(res);
    std::fclose(frames);
    std::printf("coverage 0x%016llx of %d bits\n", (unsigned long long)pbsz::g_cov2, (int)pbsz::K_NBITS);
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("zstd-checksum-ok\n");
    return 0;
}
