// The CPU build of pbs_plus_amd/csrc/zstd_decode.h under AddressSanitizer + UBSan (tests/test_zstd_core_native.py):
// every fixture frame decoded bit-exact into a guarded room, the coverage bitmap of the format branches, and every fixture
// frame through truncations, single-byte mutations and a room one byte too small. Every call has to return a status and
// leave the guards alone. One line per decode goes to the results file, so that the Python side can set the mutated
// frames against libzstd where it loads: case, kind, parameter, status, bytes decoded, their CRC-32.
//
// usage: test_zstd_core <cases file> <results file> <stride> <first>   (cases first, first + stride, ...: the test runs
// a few of these side by side)
// cases file: u32 count, then per case: u32 name length, name, u8 expected status, u64 frame length, frame,
//             u64 content length, content. Little-endian, written by the test from tests/golden/zstd_v1*.npz.
#define PBSGPU_ZSTD_COVERAGE 1
#include "../../pbs_plus_amd/csrc/zstd_decode.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr size_t kGuard = 64;
constexpr uint8_t kGuardByte = 0xa5;

struct Case {
    std::string name;
    int status;
    std::vector<uint8_t> frame, content;
};

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

uint64_t splitmix(uint64_t x) {  // tests/test_zstd_core_native.py has the same three lines
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

pbsz::State g_state;
std::vector<uint8_t> g_lit(pbsz::kLitMax + 2 * kGuard);
int g_failures = 0;

// one decode of frame[0, n) into an exact heap copy (so that ASan sees a read one byte past the frame) with `room` bytes
// between two guards
int decode(const uint8_t *frame, size_t n, size_t room, std::vector<uint8_t> &out, uint32_t *decoded) {
    std::vector<uint8_t> src(frame, frame + n);
    out.assign(room + 2 * kGuard, kGuardByte);
    std::memset(g_lit.data(), kGuardByte, kGuard);
    std::memset(g_lit.data() + kGuard + pbsz::kLitMax, kGuardByte, kGuard);
    const int st = pbsz::decode_frame<pbsz::HostLanes>(g_state, src.data(), (uint32_t)n, out.data() + kGuard, (uint32_t)room, g_lit.data() + kGuard, decoded);
    for (size_t i = 0; i < kGuard; ++i)
        if (out[i] != kGuardByte || out[kGuard + room + i] != kGuardByte || g_lit[i] != kGuardByte ||
            g_lit[kGuard + pbsz::kLitMax + i] != kGuardByte) {
            std::printf("FAIL: a guard byte was overwritten\n");
            ++g_failures;
            break;
        }
    if (st < 0 || st > 3 || (st != pbsz::OK && *decoded != 0) || *decoded > room) {
        std::printf("FAIL: status %d decoded %llu room %zu\n", st, (unsigned long long)*decoded, room);
        ++g_failures;
    }
    return st;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const size_t stride = (size_t)std::atoi(argv[3]), first = (size_t)std::atoi(argv[4]);
    if (stride == 0) return 2;
    crc_init();
    FILE *f = std::fopen(argv[1], "rb");
    FILE *res = std::fopen(argv[2], "w");
    if (!f || !res) return 2;
    uint32_t count = 0;
    if (!read_exact(f, &count, 4)) return 2;
    std::vector<Case> cases(count);
    for (Case &c : cases) {
        uint32_t nl = 0;
        uint8_t st = 0;
        uint64_t fl = 0, cl = 0;
        if (!read_exact(f, &nl, 4)) return 2;
        c.name.resize(nl);
        if (!read_exact(f, &c.name[0], nl) || !read_exact(f, &st, 1) || !read_exact(f, &fl, 8)) return 2;
        c.frame.resize(fl);
        if (!read_exact(f, c.frame.data(), fl) || !read_exact(f, &cl, 8)) return 2;
        c.content.resize(cl);
        if (!read_exact(f, c.content.data(), cl)) return 2;
        c.status = st;
    }
    std::fclose(f);

    std::vector<uint8_t> out;
    uint32_t decoded = 0;
    // 1. every fixture, bit-exact, into a room of exactly its size (and, for the frames nobody may accept, 64 KiB)
    for (size_t ci = first; ci < cases.size(); ci += stride) {
        const Case &c = cases[ci];
        const size_t room = c.status == pbsz::OK ? c.content.size() : (64u << 10);
        const int st = decode(c.frame.data(), c.frame.size(), room, out, &decoded);
        const bool same = st != pbsz::OK || (decoded == c.content.size() && (decoded == 0 || std::memcmp(out.data() + kGuard, c.content.data(), decoded) == 0));
        if (st != c.status || !same) {
            std::printf("FAIL: %s: status %d (expected %d), decoded %llu of %zu, bytes %s\n", c.name.c_str(), st, c.status,
                        (unsigned long long)decoded, c.content.size(), same ? "equal" : "DIFFER");
            ++g_failures;
        }
        std::fprintf(res, "%zu fixture 0 %d %llu %u\n", ci, st, (unsigned long long)decoded, crc32(out.data() + kGuard, decoded));
    }
    std::printf("coverage 0x%016llx of %d bits\n", (unsigned long long)pbsz::g_cov, (int)pbsz::C_NBITS);
    // 2. the mutations
    for (size_t ci = first; ci < cases.size(); ci += stride) {
        const Case &c = cases[ci];
        const size_t n = c.frame.size();
        const size_t room = c.status == pbsz::OK ? c.content.size() : (64u << 10);
        std::vector<size_t> cuts;
        for (size_t l = 0; l <= 64 && l < n; ++l) cuts.push_back(l);
        for (uint64_t j = 0; j < 97 && n; ++j) cuts.push_back(splitmix(ci * 1000003ull + j) % n);
        for (size_t l : cuts) {
            const int st = decode(c.frame.data(), l, room, out, &decoded);
            std::fprintf(res, "%zu cut %zu %d %llu %u\n", ci, l, st, (unsigned long long)decoded, crc32(out.data() + kGuard, decoded));
        }
        std::vector<uint8_t> m(c.frame);
        for (uint64_t j = 0; j < 2000 && n; ++j) {
            const uint64_t r = splitmix((ci << 32) + j + 77);
            const size_t at = r % n;
            const uint8_t old = m[at];
            m[at] = old ^ (uint8_t)(1 + (r >> 32) % 255);
            const int st = decode(m.data(), n, room, out, &decoded);
            std::fprintf(res, "%zu mut %llu %d %llu %u\n", ci, (unsigned long long)j, st, (unsigned long long)decoded,
                         crc32(out.data() + kGuard, decoded));
            m[at] = old;
        }
        if (c.status == pbsz::OK && room > 0) {
            const int st = decode(c.frame.data(), n, room - 1, out, &decoded);
            if (st != pbsz::BAD_SIZE) {
                std::printf("FAIL: %s into a room one byte too small: status %d\n", c.name.c_str(), st);
                ++g_failures;
            }
            std::fprintf(res, "%zu small 0 %d 0 0\n", ci, st);
        }
    }
    std::fclose(res);
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("zstd-core-ok\n");
    return 0;
}
