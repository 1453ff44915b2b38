// The CPU build of pbs_plus_amd/csrc/zstd_encode.h under AddressSanitizer + UBSan, in BOTH modes of the sequences section:
// mode 0, predefined tables and explicit offsets (enc::State), and mode 1, per-block tables and repeat codes (enc::TState)
// (tests/test_zstd_encode_tables_native.py). For every case and mode: the content encoded with the host policy into a room of exactly encode_bound(n) between guards, the frame
// decoded again with zstd_decode.h and compared, its length set against the bound, and the encode repeated into a room one
// byte shorter than the frame and into a room of 0, which must report BAD_SIZE and leave the guards alone. Source, room
// and every scratch buffer are heap blocks of exactly the stated size, so that ASan sees a byte read or written outside.
//
// usage: test_zstd_encode_tables <cases file> <frames file> <results file>
// cases file:   u32 count, then per case u32 name length, name, u64 content length, content (little endian)
// frames file:  per case, mode 0 then mode 1: u64 frame length, frame
// results file: per case and mode "index mode frame_length coverage_of_this_run literals_of_last_block sequences_of_last_block"
#define PBSGPU_ZSTD_COVERAGE 1
#include "../../pbs_plus_amd/csrc/zstd_encode.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr size_t kGuard = 64;
constexpr uint8_t kGuardByte = 0xa5;
namespace ze = pbsz::enc;

struct Case {
    std::string name;
    std::vector<uint8_t> content;
};

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

ze::State g_enc0;
ze::TState g_enc1;
pbsz::State g_dec;
int g_mode = 0;
int g_failures = 0;

// one encode of c into `room` bytes between two guards; out = guard, room, guard
int encode(const std::vector<uint8_t> &c, size_t room, std::vector<uint8_t> &out, uint64_t *flen) {
    std::vector<uint8_t> src(c), blk(pbsz::kBlockMax), lit(pbsz::kBlockMax);
    std::vector<uint64_t> seqs(ze::kSeqCap);
    out.assign(room + 2 * kGuard, kGuardByte);
    const int st = g_mode ? ze::encode_frame<ze::HostLanes>(g_enc1, src.data(), (uint32_t)src.size(), out.data() + kGuard, room,
                                                            blk.data(), lit.data(), seqs.data(), flen)
                          : ze::encode_frame<ze::HostLanes>(g_enc0, src.data(), (uint32_t)src.size(), out.data() + kGuard, room,
                                                            blk.data(), lit.data(), seqs.data(), flen);
    for (size_t i = 0; i < kGuard; ++i)
        if (out[i] != kGuardByte || out[kGuard + room + i] != kGuardByte) {
            std::printf("FAIL: a guard byte was overwritten (room %zu)\n", room);
            ++g_failures;
            break;
        }
    return st;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    FILE *frames = std::fopen(argv[2], "wb");
    FILE *res = std::fopen(argv[3], "w");
    if (!f || !frames || !res) return 2;
    uint32_t count = 0;
    if (!read_exact(f, &count, 4)) return 2;
    std::vector<Case> cases(count);
    for (Case &c : cases) {
        uint32_t nl = 0;
        uint64_t cl = 0;
        if (!read_exact(f, &nl, 4)) return 2;
        c.name.resize(nl);
        if (!read_exact(f, &c.name[0], nl) || !read_exact(f, &cl, 8)) return 2;
        c.content.resize(cl);
        if (!read_exact(f, c.content.data(), cl)) return 2;
    }
    std::fclose(f);

    uint64_t cov_all = 0;
    std::vector<uint8_t> out, small, back, declit(pbsz::kLitMax);
    for (size_t cm = 0; cm < 2 * cases.size(); ++cm) {
        const size_t ci = cm / 2;
        g_mode = (int)(cm & 1);
        const Case &c = cases[ci];
        const size_t n = c.content.size();
        const uint64_t bound = ze::encode_bound(n);
        uint64_t flen = 0, flen2 = 0;
        ze::g_cov = 0;
        const int st = encode(c.content, bound, out, &flen);
        const uint64_t cov = ze::g_cov;
        cov_all |= cov;
        if (st != pbsz::OK || flen == 0 || flen > bound) {
            std::printf("FAIL: %s mode %d: status %d, frame %llu, bound %llu\n", c.name.c_str(), g_mode, st, (unsigned long long)flen,
                        (unsigned long long)bound);
            ++g_failures;
            flen = 0;
        }
        // the frame through the decoder, from an exact heap copy into an exact room
        std::vector<uint8_t> frame(out.begin() + kGuard, out.begin() + kGuard + flen);
        back.assign(n, 0);
        uint32_t decoded = 0;
        const int ds = flen ? pbsz::decode_frame<pbsz::HostLanes>(g_dec, frame.data(), (uint32_t)flen, back.data(), (uint32_t)n,
                                                                  declit.data(), &decoded)
                            : pbsz::BAD_FRAME;
        if (ds != pbsz::OK || decoded != n || (n && std::memcmp(back.data(), c.content.data(), n) != 0)) {
            std::printf("FAIL: %s mode %d: decodes with status %d to %u of %zu bytes\n", c.name.c_str(), g_mode, ds, decoded, n);
            ++g_failures;
        }
        const uint64_t rooms[2] = {flen ? flen - 1 : 0, 0};
        for (uint64_t room : rooms) {
            const int s2 = encode(c.content, room, small, &flen2);
            if (s2 != pbsz::BAD_SIZE) {
                std::printf("FAIL: %s mode %d into a room of %llu: status %d\n", c.name.c_str(), g_mode, (unsigned long long)room, s2);
                ++g_failures;
            }
        }
        std::fwrite(&flen, 8, 1, frames);
        std::fwrite(frame.data(), 1, frame.size(), frames);
        const ze::State &e = g_mode ? g_enc1 : g_enc0;
        std::fprintf(res, "%zu %d %llu 0x%llx %u %u\n", ci, g_mode, (unsigned long long)flen, (unsigned long long)cov, e.nlit, e.nseq);
    }
    std::fclose(frames);
    std::fclose(res);
    std::printf("coverage 0x%016llx of %d bits\n", (unsigned long long)cov_all, (int)ze::E_NBITS_TABLES);
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("zstd-encode-tables-ok\n");
    return 0;
}
