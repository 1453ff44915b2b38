// The CPU build of pbs_plus_amd/csrc/zstd_encode.h under AddressSanitizer + UBSan with BOTH match finders: the one that
// never leaves its block (enc::State, enc::TState: window 0) and the long-range one (enc::WState, enc::WTState: window log
// 17 and 19), each without and with per-block sequence tables (tests/test_zstd_encode_window_native.py). For every case
// and mode: the content encoded with the host policy into a room of exactly encode_bound(n) between guards, the frame
// decoded again with zstd_decode.h and compared, its length set against the bound, and the encode repeated into a room one
// byte shorter than the frame and into a room of 0, which must report BAD_SIZE and leave the guards alone. In the window
// modes the content is also encoded from two parts (enc::Src2), split at several places, which must give the same frame.
// Source, room, the match finder's table and every scratch buffer are heap blocks of exactly the stated size, so that
// ASan sees a byte read or written outside.
//
// usage: test_zstd_encode_window <cases file> <frames file> <results file>
// cases file:   u32 count, then per case u32 name length, name, u64 content length, content (little endian)
// frames file:  per case and mode, in the order of kModes: u64 frame length, frame
// results file: per case and mode "index window_log tables frame_length coverage_of_this_run literals_of_last_block
//               sequences_of_last_block"
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
struct Mode {
    uint32_t window_log, tables;
};
constexpr Mode kModes[] = {{0, 0}, {0, 1}, {17, 0}, {17, 1}, {19, 0}, {19, 1}};
constexpr size_t kNModes = sizeof(kModes) / sizeof(kModes[0]);

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

ze::State g_s;
ze::TState g_t;
ze::WState g_w;
ze::WTState g_wt;
pbsz::State g_dec;
int g_failures = 0;

// one encode of c, which lies in one part (split >= its length) or in two, into `room` bytes between two guards;
// out = guard, room, guard
int encode(const Mode &m, const std::vector<uint8_t> &c, size_t split, size_t room, std::vector<uint8_t> &out, uint64_t *flen) {
    const uint32_t n = (uint32_t)c.size();
    std::vector<uint8_t> blk(pbsz::kBlockMax), lit(pbsz::kBlockMax);
    std::vector<uint64_t> seqs(ze::kSeqCap);
    out.assign(room + 2 * kGuard, kGuardByte);
    uint8_t *dst = out.data() + kGuard;
    int st;
    if (m.window_log) {
        const size_t a = split < c.size() ? split : c.size();
        std::vector<uint8_t> p0(c.begin(), c.begin() + a), p1(c.begin() + a, c.end());
        std::vector<uint32_t> tab(1u << ze::kWindowHashLog, 0xdeadbeefu);
        const ze::Src2 src{p0.data(), p1.data(), (uint32_t)a};
        st = m.tables ? ze::encode_frame<ze::HostLanes>(g_wt, src, n, dst, room, blk.data(), lit.data(), seqs.data(), flen, m.window_log, tab.data())
                      : ze::encode_frame<ze::HostLanes>(g_w, src, n, dst, room, blk.data(), lit.data(), seqs.data(), flen, m.window_log, tab.data());
    } else {
        std::vector<uint8_t> src(c);
        st = m.tables ? ze::encode_frame<ze::HostLanes>(g_t, src.data(), n, dst, room, blk.data(), lit.data(), seqs.data(), flen)
                      : ze::encode_frame<ze::HostLanes>(g_s, src.data(), n, dst, room, blk.data(), lit.data(), seqs.data(), flen);
    }
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
    size_t splits = 0;
    std::vector<uint8_t> out, small, back, declit(pbsz::kLitMax);
    for (size_t cm = 0; cm < kNModes * cases.size(); ++cm) {
        const size_t ci = cm / kNModes;
        const Mode m = kModes[cm % kNModes];
        const Case &c = cases[ci];
        const size_t n = c.content.size();
        const uint64_t bound = ze::encode_bound(n);
        uint64_t flen = 0, flen2 = 0;
        ze::g_cov = 0;
        const int st = encode(m, c.content, n, bound, out, &flen);
        const uint64_t cov = ze::g_cov;
        cov_all |= cov;
        if (st != pbsz::OK || flen == 0 || flen > bound) {
            std::printf("FAIL: %s window %u tables %u: status %d, frame %llu, bound %llu\n", c.name.c_str(), m.window_log, m.tables, st,
                        (unsigned long long)flen, (unsigned long long)bound);
            ++g_failures;
            flen = 0;
        }
        const ze::State &e = m.window_log ? (m.tables ? (const ze::State &)g_wt : g_w) : (m.tables ? (const ze::State &)g_t : g_s);
        const uint32_t nlit = e.nlit, nseq = e.nseq;
        // the frame through the decoder, from an exact heap copy into an exact room
        std::vector<uint8_t> frame(out.begin() + kGuard, out.begin() + kGuard + flen);
        back.assign(n, 0);
        uint32_t decoded = 0;
        const int ds = flen ? pbsz::decode_frame<pbsz::HostLanes>(g_dec, frame.data(), (uint32_t)flen, back.data(), (uint32_t)n,
                                                                  declit.data(), &decoded)
                            : pbsz::BAD_FRAME;
        if (ds != pbsz::OK || decoded != n || (n && std::memcmp(back.data(), c.content.data(), n) != 0)) {
            std::printf("FAIL: %s window %u tables %u: decodes with status %d to %u of %zu bytes\n", c.name.c_str(), m.window_log,
                        m.tables, ds, decoded, n);
            ++g_failures;
        }
        const uint64_t rooms[2] = {flen ? flen - 1 : 0, 0};
        for (uint64_t room : rooms) {
            const int s2 = encode(m, c.content, n, room, small, &flen2);
            if (s2 != pbsz::BAD_SIZE) {
                std::printf("FAIL: %s window %u tables %u into a room of %llu: status %d\n", c.name.c_str(), m.window_log, m.tables,
                            (unsigned long long)room, s2);
                ++g_failures;
            }
        }
        // the same content in two parts: the seam in a block's history, on a block's edge, inside a block, at either end
        if (m.window_log == 17 && n >= 2 && n <= 400000) {
            const size_t at[] = {1, n / 3, pbsz::kBlockMax - 2, pbsz::kBlockMax, pbsz::kBlockMax + 31, n - 1};
            for (size_t a : at) {
                if (a == 0 || a >= n || (n > 70000 && m.tables && a != pbsz::kBlockMax - 2)) continue;
                const int s3 = encode(m, c.content, a, bound, small, &flen2);
                ++splits;
                if (s3 != st || flen2 != flen || std::memcmp(small.data(), out.data(), out.size()) != 0) {
                    std::printf("FAIL: %s window %u tables %u in two parts split at %zu: status %d, frame %llu, or other bytes\n",
                                c.name.c_str(), m.window_log, m.tables, a, s3, (unsigned long long)flen2);
                    ++g_failures;
                }
            }
        }
        std::fwrite(&flen, 8, 1, frames);
        std::fwrite(frame.data(), 1, frame.size(), frames);
        std::fprintf(res, "%zu %u %u %llu 0x%llx %u %u\n", ci, m.window_log, m.tables, (unsigned long long)flen, (unsigned long long)cov,
                     nlit, nseq);
    }
    std::fclose(frames);
    std::fclose(res);
    std::printf("coverage 0x%016llx of %d bits\n", (unsigned long long)cov_all, (int)ze::E_NBITS_WINDOW);
    std::printf("two-part encodes %zu\n", splits);
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("zstd-encode-window-ok\n");
    return 0;
}
